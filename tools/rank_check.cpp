// rank_check.cpp -- the ranking kernels' logic (csrc/gft_rank_piece.hpp, run on the host by score_docs_host, top_docs_host and
// gather_docs_host) against naive forms written here, under the address and undefined-behaviour sanitizers: a stand-alone program,
// CPU only.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I. tools/rank_check.cpp \
//       gofindthem_amd/csrc/rank_host.cpp gofindthem_amd/csrc/select_host.cpp -o build/rank_check
//   build/rank_check 300
//
// Every input and output lies in a heap block of exactly its size -- the offsets, the entries [0, off[n]) with poison in front of
// off[0], the weights, the scores, the two top arrays of k words, the gather's blob, list and outputs --, so a read outside them or a
// store outside an output is an error of the sanitizer.  First the border cases: one document of S - 1, S, S + 1 entries (S the
// entries of a step), of B - 1, B, B + 1 (B the large path's threshold), large documents between small ones and back to back, empty
// documents everywhere, pairs that meet in the set, n_terms round the weights' and the bitset's LDS limits, weights of 2^32 - 1 whose
// sum passes 2^32; the top list at k = 1, 63, 64, 65, 4096 with fewer, as many and more documents, ties at the threshold in every
// tile, keys that differ in one digit only; the gather with repeats, empty documents and every cap.  Then N seeded random rounds of
// each, and the refusals, which must leave every output untouched.
// Exit code 0: walks and naive forms agree everywhere.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <numeric>
#include <random>
#include <set>
#include <vector>

#include "gofindthem_amd/csrc/gft_rank.hpp"

using namespace gft;

namespace {

std::mt19937_64 rng;
uint64_t rnd(uint64_t n) { return n ? rng() % n : 0; }
int failures = 0, cases = 0;

template <class T>
std::unique_ptr<T[]> exact(const std::vector<T>& v) {
    std::unique_ptr<T[]> p(new T[v.size() ? v.size() : 1]);
    std::copy(v.begin(), v.end(), p.get());
    return p;
}

void fail(const char* what, const char* name, int rc) {
    std::printf("FAIL %s: %s (rc %d)\n", what, name, rc);
    failures++;
}

typedef std::vector<std::vector<uint32_t>> Docs;
constexpr uint64_t kPat = 0xA5A5A5A5A5A5A5A5ull;

// ---- scores ---------------------------------------------------------------------------------------------------------------------
void score_case(const char* name, const Docs& D, uint32_t n_terms, uint64_t lead, const std::vector<uint32_t>* weights) {
    cases++;
    std::vector<uint64_t> off(D.size() + 1, lead);
    std::vector<uint32_t> term(lead, 0xFFFFFFFFu);
    for (size_t d = 0; d < D.size(); d++) { term.insert(term.end(), D[d].begin(), D[d].end()); off[d + 1] = term.size(); }
    auto p_off = exact(off);
    auto p_term = exact(term);
    auto p_w = exact(weights ? *weights : std::vector<uint32_t>());
    for (uint32_t flags : {0u, GFT_SCORE_DISTINCT}) {
        std::vector<uint64_t> want(D.size(), 0);
        uint64_t want_max = 0;
        for (size_t d = 0; d < D.size(); d++) {
            std::set<uint32_t> seen;
            for (uint32_t t : D[d])
                if (!flags || seen.insert(t).second) want[d] += weights ? (*weights)[t] : 1u;
            want_max = std::max(want_max, want[d]);
        }
        auto score = exact(std::vector<uint64_t>(D.size(), kPat));
        uint64_t mx = 77;
        const int rc = score_docs_host(D.empty() ? nullptr : p_off.get(), p_term.get(), D.size(), n_terms, weights ? p_w.get() : nullptr, flags, score.get(), &mx);
        bool ok = rc == GFT_OK && mx == want_max;
        for (size_t d = 0; ok && d < D.size(); d++) ok = score[d] == want[d];
        if (!ok) fail("score", name, rc);
    }
}

void score_refusals(const Docs& D, uint32_t n_terms) {
    std::vector<uint64_t> off(D.size() + 1, 0);
    std::vector<uint32_t> term;
    for (size_t d = 0; d < D.size(); d++) { term.insert(term.end(), D[d].begin(), D[d].end()); off[d + 1] = term.size(); }
    if (term.empty() || D.size() < 3) return;
    for (int kind = 0; kind < 4; kind++) {
        auto o = off;
        auto t = term;
        if (kind == 0) t[rnd(t.size())] = n_terms;
        if (kind == 1) t[rnd(2) ? 0 : t.size() - 1] = 0xFFFFFFFFu;
        if (kind == 2) { const size_t d = 1 + rnd(D.size() - 1); o[d] = o[d + 1] + 1; }
        auto p_off = exact(o);
        auto p_term = exact(t);
        auto score = exact(std::vector<uint64_t>(D.size(), kPat));
        uint64_t mx = 77;
        const int rc = score_docs_host(p_off.get(), p_term.get(), D.size(), n_terms, nullptr, kind == 3 ? 2u : (uint32_t)rnd(2), score.get(), &mx);
        bool ok = rc == GFT_E_INVALID && mx == 77;
        for (size_t d = 0; ok && d < D.size(); d++) ok = score[d] == kPat;
        if (!ok) fail("score refusal", "kind", rc);
    }
}

std::vector<uint32_t> two(uint64_t n, uint32_t a, uint32_t b) {
    std::vector<uint32_t> v(n);
    for (uint64_t i = 0; i < n; i++) v[i] = i & 1 ? b : a;
    return v;
}

std::vector<uint32_t> zipf(uint64_t n, uint32_t n_terms) {
    std::vector<uint32_t> v(n);
    for (auto& t : v) {
        const double u = (double)(rng() >> 11) / 9007199254740992.0;
        t = (uint32_t)std::min<double>(n_terms - 1, (1.0 / (1.0 - u * 0.999) - 1.0));
        if (!rnd(4)) t = (uint32_t)rnd(n_terms);
    }
    return v;
}

std::vector<uint32_t> random_weights(uint32_t n_terms) {
    std::vector<uint32_t> w(n_terms);
    for (auto& x : w) x = rnd(5) ? (uint32_t)rnd(1000) : rnd(2) ? 0u : 0xFFFFFFFFu;
    return w;
}

void score_borders() {
    const uint32_t S = kStatsStep, B = kStatsLarge, SS = kStatsSetSlots, LT = kStatsBitsetLdsTerms, WL = kRankWeightLdsTerms;
    const std::vector<uint32_t> w11 = random_weights(11), big(6, 0xFFFFFFFFu), zero(9, 0);
    for (uint32_t n : {S - 1, S, S + 1}) {
        std::vector<uint32_t> d(n);
        for (uint32_t i = 0; i < n; i++) d[i] = i % 7;
        score_case("one document", Docs{d}, 11, 0, &w11);
        Docs many((size_t)n / 5, std::vector<uint32_t>{1, 2, 3, 2, 1});
        if (n % 5) many.push_back(std::vector<uint32_t>(n % 5, 4));
        for (int k = 0; k < 30; k++) many.push_back({0, 5, 5});
        score_case("step sum", many, 11, 3, &w11);
    }
    for (uint32_t n : {B - 1, B, B + 1}) score_case("two terms", Docs{two(n, 1, 4)}, 6, 0, &big);
    score_case("large between small", Docs{{1, 2}, {}, two(B + 17, 0, 3), {2, 2}, {}}, 6, 5, &big);
    score_case("two large", Docs{two(B + 3, 0, 3), two(2 * S + 5, 1, 3)}, 6, 0, nullptr);
    score_case("empty batch", Docs(2 * kStatsStepDocs + 1), 3, 0, nullptr);
    score_case("no documents", Docs{}, 3, 0, nullptr);
    score_case("no terms", Docs(2), 0, 0, nullptr);
    score_case("weights zero", Docs{{1, 2, 8}, two(B + 1, 0, 3), {}}, 9, 2, &zero);
    score_case("set collide", Docs(200, {5, 5 + SS, 5 + 2 * SS, 5}), 3 * SS, 0, nullptr);
    for (uint32_t nt : {LT - 1, LT, LT + 1, WL - 1, WL, WL + 1}) {
        auto d = two(B + 9, 1, 4);
        for (size_t i = 5; i < d.size(); i += 7) d[i] = nt - 1;
        const auto w = random_weights(nt);
        score_case("lds limits", Docs{{0, nt - 1}, d, {nt - 1, 0, nt - 1}}, nt, 0, &w);
    }
    Docs r;
    for (uint32_t k = 0; k < (kStatsRangeWeight - 20) / 8; k++) r.push_back({1, 2, 3, 4, 5, 6, 7});
    r.push_back(two(B + 5, 1, 4));
    for (uint32_t k = 0; k < kStatsRangeWeight / 2; k++) r.push_back({7, 7, 1, 0, 2, 7, 7});
    const auto w9 = random_weights(9);
    score_case("ranges", r, 9, 11, &w9);
}

// ---- the top list ---------------------------------------------------------------------------------------------------------------
void top_case(const char* name, const std::vector<uint64_t>& score, uint32_t k, uint64_t doc_base) {
    cases++;
    std::vector<uint64_t> order;
    for (uint64_t d = 0; d < score.size(); d++)
        if (score[d]) order.push_back(d);
    std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return score[a] != score[b] ? score[a] > score[b] : a < b; });
    if (order.size() > k) order.resize(k);
    auto p_score = exact(score);
    auto ti = exact(std::vector<uint64_t>(k, kPat)), ts = exact(std::vector<uint64_t>(k, kPat + 1));
    uint64_t n = 77;
    const int rc = top_docs_host(score.empty() ? nullptr : p_score.get(), score.size(), k, doc_base, ti.get(), ts.get(), &n);
    bool ok = rc == GFT_OK && n == order.size();
    for (size_t r = 0; ok && r < k; r++)
        ok = r < n ? (ti[r] == doc_base + order[r] && ts[r] == score[order[r]]) : (ti[r] == kPat && ts[r] == kPat + 1);
    if (!ok) fail("top", name, rc);
}

void top_borders() {
    const uint32_t PT = kRankPlaceTile, K = kRankMaxK;
    for (uint32_t k : {1u, 63u, 64u, 65u, K})
        for (uint64_t n : {(uint64_t)k - 1, (uint64_t)k, (uint64_t)k + 1, (uint64_t)3 * k + 7}) {
            std::vector<uint64_t> s(n);
            for (auto& v : s) v = rnd(40);
            top_case("k and n", s, k, 1ull << 41);
        }
    top_case("all equal", std::vector<uint64_t>(3 * PT + 5, 9), PT + 1, 0);
    top_case("all zero", std::vector<uint64_t>(2 * PT + 1, 0), 64, 0);
    {
        std::vector<uint64_t> s(5 * PT + 77, 3);
        for (size_t i = 0; i < s.size(); i += 50) s[i] = 7;
        for (uint64_t i : {5u, PT - 1, PT, 2 * PT + 1, 4 * PT}) s[i] = 100 + i;
        for (uint32_t k : {4u, 5u, 6u, 64u, 300u}) top_case("shared threshold", s, k, 3);
    }
    {
        std::vector<uint64_t> lo(2 * PT + 9), hi(2 * PT + 9), ex;
        for (auto& v : lo) v = 0x0123456789ABCD00ull + rnd(256);
        for (auto& v : hi) v = (1 + rnd(200)) << 56;
        for (int i = 0; i < 30; i++)
            for (unsigned long long v : {~0ull, 1ull << 32, (1ull << 32) - 1, (1ull << 32) + 1, 0ull, ~0ull - 1, 1ull << 63}) ex.push_back(v);
        for (uint32_t k : {1u, 64u, 700u}) { top_case("lowest digit", lo, k, 0); top_case("highest digit", hi, k, 0); top_case("extremes", ex, k, ~0ull >> 8); }
    }
    top_case("k zero", {4, 5, 6}, 0, 0);
    auto ti = exact(std::vector<uint64_t>(K + 1, kPat)), ts = exact(std::vector<uint64_t>(K + 1, kPat));
    const std::vector<uint64_t> s(K + 9, 1);
    uint64_t n = 77;
    const int rc = top_docs_host(s.data(), s.size(), K + 1, 0, ti.get(), ts.get(), &n);
    if (rc != GFT_E_INVALID || ti[0] != kPat || ts[K] != kPat) fail("top refusal", "k above the limit", rc);
}

// ---- the gather -----------------------------------------------------------------------------------------------------------------
void gather_case(const char* name, const std::vector<uint32_t>& lens, const std::vector<uint64_t>& list, uint64_t idx_base, uint64_t lead) {
    cases++;
    std::vector<uint64_t> off(lens.size() + 1, lead);
    for (size_t d = 0; d < lens.size(); d++) off[d + 1] = off[d] + lens[d];
    std::vector<uint8_t> blob(off.back());
    for (auto& b : blob) b = (uint8_t)(1 + rnd(250));
    std::vector<uint8_t> want;
    std::vector<uint64_t> want_off{0}, idx;
    for (uint64_t d : list) {
        want.insert(want.end(), blob.begin() + off[d], blob.begin() + off[d + 1]);
        want_off.push_back(want.size());
        idx.push_back(d + idx_base);
    }
    auto p_blob = exact(blob);
    auto p_off = exact(off);
    auto p_idx = exact(idx);
    for (uint64_t cap : {(uint64_t)want.size(), (uint64_t)want.size() - (want.empty() ? 0 : 1), (uint64_t)want.size() / 2, (uint64_t)0, (uint64_t)want.size() + 5}) {
        auto out = exact(std::vector<uint8_t>(cap, 0xA5));
        auto out_off = exact(std::vector<uint64_t>(list.size() + 1, kPat));
        uint64_t total = 77;
        const int rc = gather_docs_host(p_blob.get(), p_off.get(), lens.size(), list.empty() ? nullptr : p_idx.get(), list.size(), idx_base, cap ? out.get() : nullptr,
                                        cap, out_off.get(), &total);
        bool ok = rc == GFT_OK && total == want.size();
        for (size_t j = 0; ok && j <= list.size(); j++) ok = out_off[j] == want_off[j];
        for (uint64_t p = 0; ok && p < cap; p++) ok = out[p] == (p < want.size() ? want[p] : 0xA5);
        if (!ok) fail("gather", name, rc);
    }
    if (list.empty()) return;
    for (uint64_t bad : {(uint64_t)lens.size() + idx_base, (uint64_t)~0ull, idx_base - 1}) {
        if (bad == idx_base - 1 && !idx_base) continue;
        auto ix = idx;
        ix[rnd(ix.size())] = bad;
        auto p_bad = exact(ix);
        auto out = exact(std::vector<uint8_t>(64, 0xA5));
        auto out_off = exact(std::vector<uint64_t>(list.size() + 1, kPat));
        uint64_t total = 77;
        const int rc = gather_docs_host(p_blob.get(), p_off.get(), lens.size(), p_bad.get(), list.size(), idx_base, out.get(), 64, out_off.get(), &total);
        bool ok = rc == GFT_E_INVALID && out_off[0] == kPat && out_off[list.size()] == kPat;
        for (int p = 0; ok && p < 64; p++) ok = out[p] == 0xA5;
        if (!ok) fail("gather refusal", name, rc);
    }
}

void gather_borders() {
    const std::vector<uint32_t> lens{0, 1, kSelChunk - 1, kSelChunk, kSelChunk + 1, 0, 0, kSelTrip - 1, kSelTrip, kSelTrip + 1, 3, kSelTile - 1, kSelTile,
                                     kSelTile + 1, 0, 2 * kSelTile + 5, 7, 0};
    std::vector<uint64_t> ident(lens.size());
    std::iota(ident.begin(), ident.end(), 0);
    gather_case("identity", lens, ident, 0, 9);
    gather_case("reversed", lens, std::vector<uint64_t>(ident.rbegin(), ident.rend()), 1ull << 40, 9);
    gather_case("repeats", lens, {3, 3, 3, 15, 0, 15, 3, 8, 8}, 7, 0);
    gather_case("empty list", lens, {}, 0, 3);
    gather_case("zero-byte documents", lens, {0, 5, 6, 14, 17}, 0, 3);
}

}  // namespace

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? std::atoi(argv[1]) : 100;
    rng.seed(20261021);
    score_borders();
    top_borders();
    gather_borders();
    const int fixed = cases;
    for (int it = 0; it < rounds; it++) {
        const uint32_t n_terms = (uint32_t[]){1, 3, 50, 1000, kRankWeightLdsTerms + 3}[rnd(5)];
        Docs D(rnd(it % 4 == 0 ? 3000 : 300));
        for (auto& d : D) {
            const uint64_t kind = rnd(100);
            d = zipf(kind < 2 ? kStatsStep + rnd(2 * kStatsStep) : kind < 10 ? rnd(300) : rnd(6), n_terms);
        }
        const auto w = random_weights(n_terms);
        score_case("random", D, n_terms, rnd(40), rnd(3) ? &w : nullptr);
        score_refusals(D, n_terms);
        std::vector<uint64_t> s(rnd(it % 5 ? 3000 : 20000));
        const int kind = (int)rnd(4);
        for (auto& v : s) v = kind == 0 ? rnd(8) : kind == 1 ? rng() : kind == 2 ? rnd(1ull << 20) << (8 * rnd(6)) : (rnd(3) ? 0 : rnd(1000));
        top_case("random", s, (uint32_t)(rnd(3) ? rnd(130) : rnd(kRankMaxK + 1)), rnd(2) ? rng() >> 8 : 0);
        std::vector<uint32_t> lens(1 + rnd(40));
        for (auto& l : lens) l = (uint32_t)(rnd(4) ? rnd(40) : rnd(3 * kSelTrip));
        std::vector<uint64_t> list(rnd(60));
        for (auto& d : list) d = rnd(lens.size());
        gather_case("random", lens, list, rnd(2) ? rng() >> 4 : 0, rnd(30));
    }
    std::printf("%s: %d border cases and %d random rounds, %d failures\n", failures ? "FAILED" : "ok", fixed, rounds, failures);
    return failures ? 1 : 0;
}
