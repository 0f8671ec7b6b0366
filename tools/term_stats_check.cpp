// term_stats_check.cpp -- the statistics kernels' logic (csrc/gft_stats_piece.hpp, run on the host by term_stats_host and
// count_columns_host) against a naive count written here, under the address and undefined-behaviour sanitizers: a stand-alone
// program, CPU only.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I. tools/term_stats_check.cpp \
//       gofindthem_amd/csrc/stats_host.cpp -o build/term_stats_check
//   build/term_stats_check 300
//
// Every input and output lies in a heap block of exactly its size -- the offsets, the entries [0, off[n]) with poison in front of
// off[0], the three counter arrays of n_terms words --, so a read outside them or a store outside the counters is an error of the
// sanitizer.  First the border cases: one document of S - 1, S, S + 1 entries (S the entries of a step), a document of B - 1, B,
// B + 1 entries of two terms (B the large path's threshold), large documents between small ones and back to back, empty documents
// everywhere, terms that meet in a cache slot and pairs that meet in the set, n_terms round the bitset's LDS limit.  Then N seeded
// random rounds: Zipf-like terms, documents from lines to several steps, a random lead, overwrite and accumulate with a doc_base,
// one output dropped at random; then a term id put out of range and an offset made to descend, which must be refused with every
// counter untouched.  The column count: random bitmaps with garbage above n_cols, with and without row indices.
// Exit code 0: walk and naive count agree everywhere.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <random>
#include <set>
#include <vector>

#include "gofindthem_amd/csrc/gft_stats.hpp"

using namespace gft;

namespace {

std::mt19937_64 rng;
uint64_t rnd(uint64_t n) { return n ? rng() % n : 0; }
int failures = 0;

template <class T>
std::unique_ptr<T[]> exact(const std::vector<T>& v) {
    std::unique_ptr<T[]> p(new T[v.size() ? v.size() : 1]);
    std::copy(v.begin(), v.end(), p.get());
    return p;
}

typedef std::vector<std::vector<uint32_t>> Docs;

struct Naive { std::vector<uint64_t> occ, docs, first; };

Naive naive(const Docs& D, uint32_t n_terms, uint64_t doc_base, const Naive* into) {
    Naive r;
    if (into) r = *into;
    else { r.occ.assign(n_terms, 0); r.docs.assign(n_terms, 0); r.first.assign(n_terms, ~0ull); }
    for (size_t d = 0; d < D.size(); d++) {
        std::set<uint32_t> seen;
        for (uint32_t t : D[d]) {
            r.occ[t]++;
            if (seen.insert(t).second) { r.docs[t]++; r.first[t] = std::min<uint64_t>(r.first[t], doc_base + d); }
        }
    }
    return r;
}

void run_case(const char* name, const Docs& D, uint32_t n_terms, uint64_t lead, bool accumulate, uint64_t doc_base, int drop) {
    std::vector<uint64_t> off(D.size() + 1, lead);
    std::vector<uint32_t> term(lead, 0xFFFFFFFFu);
    for (size_t d = 0; d < D.size(); d++) {
        term.insert(term.end(), D[d].begin(), D[d].end());
        off[d + 1] = term.size();
    }
    Naive start;
    start.occ.resize(n_terms); start.docs.resize(n_terms); start.first.resize(n_terms);
    for (uint32_t t = 0; t < n_terms; t++) { start.occ[t] = 0xFFFFFFF0ull + rnd(64); start.docs[t] = rnd(5); start.first[t] = rnd(3) ? ~0ull : rnd(1000); }
    const Naive want = naive(D, n_terms, doc_base, accumulate ? &start : nullptr);
    auto p_off = exact(off);
    auto p_term = exact(term);
    auto occ = exact(start.occ), docs = exact(start.docs), first = exact(start.first);
    const int rc = term_stats_host(D.empty() ? nullptr : p_off.get(), p_term.get(), D.size(), n_terms, accumulate ? GFT_STATS_ACCUMULATE : 0, doc_base,
                                   drop == 0 ? nullptr : occ.get(), drop == 1 ? nullptr : docs.get(), drop == 2 ? nullptr : first.get());
    bool ok = rc == GFT_OK;
    for (uint32_t t = 0; ok && t < n_terms; t++)
        ok = occ[t] == (drop == 0 ? start.occ[t] : want.occ[t]) && docs[t] == (drop == 1 ? start.docs[t] : want.docs[t]) &&
             first[t] == (drop == 2 ? start.first[t] : want.first[t]);
    if (!ok) { std::printf("FAIL %s (rc %d, %zu documents, %u terms)\n", name, rc, D.size(), n_terms); failures++; }
}

void run_refusals(const Docs& D, uint32_t n_terms) {
    std::vector<uint64_t> off(D.size() + 1, 0);
    std::vector<uint32_t> term;
    for (size_t d = 0; d < D.size(); d++) { term.insert(term.end(), D[d].begin(), D[d].end()); off[d + 1] = term.size(); }
    if (term.empty() || D.size() < 3) return;
    for (int kind = 0; kind < 3; kind++) {
        auto o = off;
        auto t = term;
        if (kind == 0) t[rnd(t.size())] = n_terms;
        if (kind == 1) t[rnd(2) ? 0 : t.size() - 1] = 0xFFFFFFFFu;
        if (kind == 2) { const size_t d = 1 + rnd(D.size() - 1); o[d] = o[d + 1] + 1; }   // (d < n: the offset behind it is smaller now)
        std::vector<uint64_t> pat(n_terms, 0xA5A5A5A5A5A5A5A5ull);
        auto p_off = exact(o);
        auto p_term = exact(t);
        auto a = exact(pat), b = exact(pat), c = exact(pat);
        const int rc = term_stats_host(p_off.get(), p_term.get(), D.size(), n_terms, rnd(2) ? GFT_STATS_ACCUMULATE : 0, 7, a.get(), b.get(), c.get());
        bool ok = rc == GFT_E_INVALID;
        for (uint32_t k = 0; ok && k < n_terms; k++) ok = a[k] == pat[k] && b[k] == pat[k] && c[k] == pat[k];
        if (!ok) { std::printf("FAIL refusal %d (rc %d)\n", kind, rc); failures++; }
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
        t = (uint32_t)std::min<double>(n_terms - 1, (1.0 / (1.0 - u * 0.999) - 1.0));   // heavy at 0, a long tail
        if (!rnd(4)) t = (uint32_t)rnd(n_terms);
    }
    return v;
}

void borders() {
    const uint32_t S = kStatsStep, B = kStatsLarge, CS = kStatsCacheSlots, SS = kStatsSetSlots, LT = kStatsBitsetLdsTerms;
    for (uint32_t n : {S - 1, S, S + 1}) {
        std::vector<uint32_t> d(n);
        for (uint32_t i = 0; i < n; i++) d[i] = i % 7;
        run_case("one document", Docs{d}, 11, 0, false, 0, -1);
        Docs many((size_t)n / 5, std::vector<uint32_t>{1, 2, 3, 2, 1});
        if (n % 5) many.push_back(std::vector<uint32_t>(n % 5, 4));
        for (int k = 0; k < 30; k++) many.push_back({0, 5, 5});
        run_case("step sum", many, 6, 3, false, 9, -1);
    }
    for (uint32_t n : {B - 1, B, B + 1}) run_case("two terms", Docs{two(n, 1, 4)}, 6, 0, false, 0, -1);
    run_case("large between small", Docs{{1, 2}, {}, two(B + 17, 0, 3), {2, 2}, {}}, 5, 5, false, 1, -1);
    run_case("two large", Docs{two(B + 3, 0, 3), two(2 * S + 5, 1, 3)}, 5, 0, true, 1ull << 40, -1);
    run_case("empty batch", Docs(2 * kStatsStepDocs + 1), 3, 0, false, 0, -1);
    run_case("no documents", Docs{}, 3, 0, false, 0, -1);
    run_case("cache collide", Docs(3 * S / 4, {7, 7 + CS, 7 + 2 * CS, 7}), 3 * CS, 0, false, 0, -1);
    run_case("set collide", Docs(200, {5, 5 + SS, 5 + 2 * SS, 5}), 3 * SS, 0, false, 0, -1);
    {
        std::vector<uint32_t> d(3 * S + 9);
        for (size_t i = 0; i < d.size(); i++) d[i] = (uint32_t)i;
        run_case("evict, large", Docs{d}, (uint32_t)d.size(), 0, false, 0, -1);
        Docs lines;
        for (size_t i = 0; i + 8 <= d.size(); i += 8) lines.emplace_back(d.begin() + i, d.begin() + i + 8);
        run_case("evict, lines", lines, (uint32_t)d.size(), 0, false, 0, -1);
    }
    for (uint32_t nt : {LT - 1, LT, LT + 1, LT + 70}) {
        auto d = two(B + 9, 1, 4);
        for (size_t i = 5; i < d.size(); i += 7) d[i] = nt - 1;
        run_case("bitset limit", Docs{{0, nt - 1}, d, {nt - 1, 0, nt - 1}}, nt, 0, false, 0, -1);
    }
    // several workgroups with a large document on a range's border
    Docs r;
    for (uint32_t k = 0; k < (kStatsRangeWeight - 20) / 8; k++) r.push_back({1, 2, 3, 4, 5, 6, 7});
    r.push_back(two(B + 5, 1, 4));
    for (uint32_t k = 0; k < kStatsRangeWeight / 2; k++) r.push_back({7, 7, 1, 0, 2, 7, 7});
    run_case("ranges", r, 9, 11, false, 3, -1);
}

void columns(int rounds) {
    for (int it = 0; it < rounds; it++) {
        const uint32_t n_cols = 1 + (uint32_t)rnd(it % 3 ? 70 : 200), W = stats_col_words(n_cols);
        const uint64_t rows = rnd(it % 5 ? 200 : 3 * kStatsColRows);
        std::vector<uint32_t> bm(rows * W);
        for (auto& w : bm) w = (uint32_t)rng() & (uint32_t)rng();
        std::vector<uint64_t> idx;
        const bool use_idx = rnd(2) && rows;
        if (use_idx) { idx.resize(rnd(2 * rows)); for (auto& r : idx) r = rnd(rows); }
        const uint64_t n = use_idx ? idx.size() : rows;
        std::vector<uint64_t> want(n_cols, it & 1 ? 0xFFFFFFFFull : 0), start(n_cols, 0xFFFFFFFFull);
        for (uint64_t r = 0; r < n; r++)
            for (uint32_t c = 0; c < n_cols; c++) want[c] += bm[(use_idx ? idx[r] : r) * W + c / 32] >> (c & 31) & 1u;
        auto p_bm = exact(bm);
        auto p_idx = exact(idx);
        auto count = exact(start);
        const int rc = count_columns_host(p_bm.get(), n, n_cols, use_idx ? p_idx.get() : nullptr, it & 1 ? GFT_STATS_ACCUMULATE : 0, count.get());
        bool ok = rc == GFT_OK;
        for (uint32_t c = 0; ok && c < n_cols; c++) ok = count[c] == want[c];
        if (!ok) { std::printf("FAIL columns round %d (rc %d)\n", it, rc); failures++; }
    }
}

}  // namespace

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? std::atoi(argv[1]) : 100;
    rng.seed(20261020);
    borders();
    for (int it = 0; it < rounds; it++) {
        const uint32_t n_terms = (uint32_t[]){1, 3, 50, 1000, 4 * kStatsCacheSlots + 3}[rnd(5)];
        Docs D(rnd(it % 4 == 0 ? 3000 : 300));
        for (auto& d : D) {
            const uint64_t kind = rnd(100);
            d = zipf(kind < 2 ? kStatsStep + rnd(2 * kStatsStep) : kind < 10 ? rnd(300) : rnd(6), n_terms);
        }
        run_case("random", D, n_terms, rnd(40), rnd(2), rnd(3) ? rnd(1ull << 45) : 0, (int)rnd(6) - 3);
        run_refusals(D, n_terms);
    }
    columns(rounds);
    std::printf("%s: %d border cases and %d random rounds, %d failures\n", failures ? "FAILED" : "ok", 25, rounds, failures);
    return failures ? 1 : 0;
}
