// excerpt_check.cpp -- the excerpt kernels' logic (csrc/gft_excerpt_piece.hpp, run on the host by excerpt_spans_host) against an
// independent union of intervals written here, under the address and undefined-behaviour sanitizers: a stand-alone program, CPU
// only.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I. tools/excerpt_check.cpp \
//       gofindthem_amd/csrc/excerpt_host.cpp -o build/excerpt_check
//   build/excerpt_check 300
//
// Every input and output lies in a heap block of exactly its size -- the text of doc_off[n] bytes with no slack, the span arrays,
// the output arrays of cap entries --, so a read outside them (a snap that leaves its document at the blob's ends) or a store past
// a cap is an error of the sanitizer.  N seeded random rounds, each: a random batch (empty documents, documents without spans,
// continuation bytes in runs of up to five, zero-length spans, ends ascending), random before / after (0 and 0xFFFFFFFF among
// them), the flag on or off; every few rounds more spans than a tile, and once more than a carry trip's.  Every round draws a
// span base s0, 0 among the values: span_off[0] = s0, the span arrays are blocks of exactly s0 + n entries whose first s0 hold a
// span no document could hold, span_rel is a block of s0 + n entries too, and the brute force is indexed the same way -- a walk
// that dropped a base reads the poison or stores where the brute force left the pattern.  The brute force marks,
// per document, the closed interval of every window on a grid of whole and half positions -- touching windows share a point, a
// gap of one byte leaves one unmarked -- and reads the excerpts off the runs of marked points.  The walk runs under exact caps,
// count only, and caps that cut the list and the bytes; then one span's end is put in front of its neighbour's and one span past
// its document's end, which must be refused with every output untouched.
// Exit code 0: walk and brute force agree everywhere.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "gofindthem_amd/csrc/gft_excerpt.hpp"

using namespace gft;

namespace {

std::mt19937_64 rng;
uint64_t rnd(uint64_t n) { return n ? rng() % n : 0; }

template <class T>
std::unique_ptr<T[]> exact(const std::vector<T>& v) {
    std::unique_ptr<T[]> p(new T[v.size() ? v.size() : 1]);
    for (size_t i = 0; i < v.size(); i++) p[i] = v[i];
    return p;
}

struct Batch {
    std::vector<uint8_t> text;
    std::vector<uint64_t> doc_off, span_off;
    std::vector<uint32_t> start, len;
    uint32_t before, after, flags;
    uint64_t s0 = 0;               // span_off[0]: the entries [0, s0) of start / len are poison
};

constexpr uint32_t kPoison = 0xFFFFFFFFu, kUntouched = 0xA5A5A5A5u;

struct Result {
    std::vector<uint8_t> out;
    std::vector<uint64_t> exc_off, exc_doc, exc_span_off, doc_exc_off;
    std::vector<uint32_t> exc_start, span_rel;
};

bool cont(uint8_t b) { return (b & 0xC0) == 0x80; }

// the contract, by brute force
Result brute(const Batch& B) {
    Result R;
    const uint64_t n_docs = B.doc_off.size() - 1;
    R.exc_off.push_back(0);
    R.doc_exc_off.push_back(0);
    R.span_rel.assign(B.start.size(), kUntouched);                 // (the entries below s0 are never written)
    for (uint64_t d = 0; d < n_docs; d++) {
        const uint8_t* doc = B.text.data() + B.doc_off[d];
        const uint64_t L = B.doc_off[d + 1] - B.doc_off[d];
        std::vector<uint8_t> grid(2 * L + 1, 0);
        std::vector<std::pair<uint64_t, uint64_t>> win;
        for (uint64_t s = B.span_off[d]; s < B.span_off[d + 1]; s++) {
            uint64_t lo = B.start[s] > B.before ? (uint64_t)B.start[s] - B.before : 0;
            uint64_t hi = (uint64_t)B.start[s] + B.len[s] + B.after;
            if (hi > L) hi = L;
            if (B.flags & GFT_EXCERPT_RUNES) {
                for (int k = 0; k < 3 && lo > 0 && lo < L && cont(doc[lo]); k++) lo--;
                for (int k = 0; k < 3 && hi < L && cont(doc[hi]); k++) hi++;
            }
            win.emplace_back(lo, hi);
            for (uint64_t p = 2 * lo; p <= 2 * hi; p++) grid[p] = 1;
        }
        // the runs of marked points, in order; a window belongs to the run that holds its first point
        std::vector<std::pair<uint64_t, uint64_t>> runs;
        for (uint64_t p = 0; p <= 2 * L; p++) {
            if (!grid[p]) continue;
            uint64_t q = p;
            while (q + 1 <= 2 * L && grid[q + 1]) q++;
            runs.emplace_back(p / 2, q / 2);
            p = q;
        }
        std::vector<uint64_t> first_span(runs.size(), ~0ull);
        for (uint64_t s = B.span_off[d]; s < B.span_off[d + 1]; s++) {
            const auto& w = win[s - B.span_off[d]];
            // (the runs are disjoint and ascend: the one that holds the window is the last that begins at or in front of it)
            const uint64_t r = std::upper_bound(runs.begin(), runs.end(), std::pair<uint64_t, uint64_t>(w.first, ~(uint64_t)0)) - runs.begin() - 1;
            if (!(runs[r].first <= w.first && w.second <= runs[r].second)) std::abort();
            if (first_span[r] == ~0ull) first_span[r] = s;
            R.span_rel[s] = (uint32_t)(B.start[s] - runs[r].first);
        }
        for (size_t r = 0; r < runs.size(); r++) {
            R.exc_doc.push_back(d);
            R.exc_start.push_back((uint32_t)runs[r].first);
            R.exc_span_off.push_back(first_span[r]);
            R.out.insert(R.out.end(), doc + runs[r].first, doc + runs[r].second);
            R.exc_off.push_back(R.out.size());
        }
        R.doc_exc_off.push_back(R.exc_doc.size());
    }
    R.exc_span_off.push_back(B.span_off[n_docs]);
    return R;
}

Batch random_batch(uint64_t n_docs, uint64_t max_len, uint64_t max_spans, uint64_t min_spans = 0) {
    Batch B;
    static const uint32_t reach[] = {0, 0, 1, 2, 3, 5, 9, 40, 0xFFFFFFFFu};
    B.before = reach[rnd(9)];
    B.after = reach[rnd(9)];
    B.flags = rnd(3) ? GFT_EXCERPT_RUNES : 0;
    static const uint64_t base[] = {0, 0, 1, 2, kExcTile - 1, kExcTile, kExcTile + 1, 3 * kExcTile + 7};
    B.s0 = rnd(9) < 8 ? base[rnd(8)] : rnd(1000);
    B.start.assign(B.s0, kPoison);
    B.len.assign(B.s0, kPoison);
    B.doc_off.push_back(0);
    B.span_off.push_back(B.s0);
    for (uint64_t d = 0; d < n_docs; d++) {
        const uint64_t L = rnd(5) ? rnd(max_len + 1) : 0;
        for (uint64_t i = 0; i < L; i++) {
            const uint64_t r = rnd(10);
            B.text.push_back(r < 4 ? (uint8_t)('a' + rnd(26)) : r < 8 ? (uint8_t)(0x80 + rnd(64)) : (uint8_t)rnd(256));
        }
        B.doc_off.push_back(B.text.size());
        std::vector<uint64_t> ends;
        for (uint64_t k = rnd(4) ? min_spans + rnd(max_spans - min_spans + 1) : 0; k > 0; k--) ends.push_back(rnd(L + 1));
        std::sort(ends.begin(), ends.end());
        for (uint64_t e : ends) {
            const uint64_t n = rnd(std::min<uint64_t>(e, 12) + 1);
            B.start.push_back((uint32_t)(e - n));
            B.len.push_back((uint32_t)n);
        }
        B.span_off.push_back(B.start.size());
    }
    return B;
}

int fails = 0;
void expect(bool ok, const char* what, uint64_t round) {
    if (ok) return;
    std::fprintf(stderr, "round %llu: %s\n", (unsigned long long)round, what);
    fails++;
}

// the walk under (cap_bytes, cap_exc) into blocks of exactly those sizes; compared with the brute force up to the caps
void check(const Batch& B, const Result& want, uint64_t cap_bytes, uint64_t cap_exc, uint64_t round) {
    const uint64_t n_docs = B.doc_off.size() - 1, m = want.exc_doc.size(), total = want.out.size();
    auto text = exact(B.text);
    auto doc_off = exact(B.doc_off), span_off = exact(B.span_off);
    auto start = exact(B.start), len = exact(B.len);
    std::unique_ptr<uint8_t[]> out(new uint8_t[cap_bytes ? cap_bytes : 1]);
    std::unique_ptr<uint64_t[]> exc_off(new uint64_t[cap_exc + 1]), exc_doc(new uint64_t[cap_exc ? cap_exc : 1]), exc_span_off(new uint64_t[cap_exc + 1]),
        doc_exc_off(new uint64_t[n_docs + 1]);
    std::unique_ptr<uint32_t[]> exc_start(new uint32_t[cap_exc ? cap_exc : 1]), span_rel(new uint32_t[B.start.size() ? B.start.size() : 1]);
    for (size_t s = 0; s < B.start.size(); s++) span_rel[s] = kUntouched;
    uint64_t got_m = ~0ull, got_total = ~0ull;
    const int rc = excerpt_spans_host(text.get(), doc_off.get(), n_docs, span_off.get(), start.get(), len.get(), B.before, B.after, B.flags,
                                      cap_bytes ? out.get() : nullptr, cap_bytes, exc_off.get(), cap_exc ? exc_doc.get() : nullptr,
                                      cap_exc ? exc_start.get() : nullptr, exc_span_off.get(), cap_exc, B.start.empty() ? nullptr : span_rel.get(),
                                      doc_exc_off.get(), &got_m, &got_total);
    expect(rc == GFT_OK, "the walk refuses a good batch", round);
    if (rc != GFT_OK) return;
    expect(got_m == m && got_total == total, "n_exc / total", round);
    for (uint64_t r = 0; r <= m && r <= cap_exc; r++)
        expect(exc_off[r] == want.exc_off[r] && exc_span_off[r] == want.exc_span_off[r], "exc_off / exc_span_off", round);
    for (uint64_t r = 0; r < m && r < cap_exc; r++) expect(exc_doc[r] == want.exc_doc[r] && exc_start[r] == want.exc_start[r], "exc_doc / exc_start", round);
    for (size_t s = 0; s < B.start.size(); s++) expect(span_rel[s] == want.span_rel[s], "span_rel", round);
    for (uint64_t d = 0; d <= n_docs; d++) expect(doc_exc_off[d] == want.doc_exc_off[d], "doc_exc_off", round);
    expect(!std::min(cap_bytes, total) || std::memcmp(out.get(), want.out.data(), (size_t)std::min(cap_bytes, total)) == 0, "the excerpts' bytes", round);
}

void check_refused(Batch B, uint64_t round) {
    const uint64_t n_docs = B.doc_off.size() - 1;
    std::vector<uint8_t> out(B.text.size() + 1, 0xA5);
    std::vector<uint64_t> a(B.start.size() + 2, 0xA5A5A5A5A5A5A5A5ull), b(a), c(a), deo(n_docs + 1, 0xA5A5A5A5A5A5A5A5ull);
    std::vector<uint32_t> es(B.start.size() + 1, 0xA5A5A5A5u), rel(es);
    const int rc = excerpt_spans_host(B.text.data(), B.doc_off.data(), n_docs, B.span_off.data(), B.start.data(), B.len.data(), B.before, B.after, B.flags,
                                      out.data(), out.size(), a.data(), b.data(), es.data(), c.data(), B.start.size(), rel.data(), deo.data(), nullptr,
                                      nullptr);
    expect(rc == GFT_E_INVALID, "a bad batch is not refused", round);
    bool clean = true;
    for (uint8_t x : out) clean = clean && x == 0xA5;
    for (auto* v : {&a, &b, &c, &deo})
        for (uint64_t x : *v) clean = clean && x == 0xA5A5A5A5A5A5A5A5ull;
    for (auto* v : {&es, &rel})
        for (uint32_t x : *v) clean = clean && x == 0xA5A5A5A5u;
    expect(clean, "a refused call wrote something", round);
}

}  // namespace

int main(int argc, char** argv) {
    const uint64_t rounds = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 100;
    for (uint64_t round = 0; round < rounds; round++) {
        rng.seed(1000 + round);
        Batch B;
        if (round == 7) {                                                                             // past a carry trip
            B = random_batch(60, 30000, 9000, 7000);
            B.before = std::min(B.before, 40u);                                                       // (the brute force marks every window's points)
            B.after = std::min(B.after, 40u);
        }
        else if (round % 5 == 0) B = random_batch(1 + rnd(12), 2000, 3 * kExcTile);                  // several tiles
        else B = random_batch(rnd(30), 120, 14);
        if (B.doc_off.size() == 1) {                                                                  // no documents
            uint64_t eo = 7, eso = 7, deo = 7;
            expect(excerpt_spans_host(nullptr, nullptr, 0, nullptr, nullptr, nullptr, 1, 1, 0, nullptr, 0, &eo, nullptr, nullptr, &eso, 0, nullptr, &deo,
                                      nullptr, nullptr) == GFT_OK && !eo && !eso && !deo, "no documents", round);
            const uint64_t nine = 9;                                                                  // (offsets of no document are not read)
            eo = eso = deo = 7;
            expect(excerpt_spans_host(nullptr, &nine, 0, &nine, nullptr, nullptr, 1, 1, 0, nullptr, 0, &eo, nullptr, nullptr, &eso, 0, nullptr, &deo,
                                      nullptr, nullptr) == GFT_OK && !eo && !eso && !deo, "no documents, offsets given", round);
            continue;
        }
        const Result want = brute(B);
        const uint64_t m = want.exc_doc.size(), total = want.out.size();
        if (round == 7) expect(B.start.size() - B.s0 > (uint64_t)kExcTile * kExcCarryTiles, "round 7 is to pass a carry trip", round);
        check(B, want, total, m, round);
        check(B, want, 0, 0, round);
        if (m) check(B, want, rnd(total + 1), rnd(m), round);
        // refusals: ends that descend; a span past its document's end
        for (uint64_t d = 0; d + 1 < B.doc_off.size(); d++) {
            const uint64_t L = B.doc_off[d + 1] - B.doc_off[d];
            if (B.span_off[d + 1] - B.span_off[d] >= 2) {
                Batch bad = B;
                const uint64_t s = B.span_off[d] + 1 + rnd(B.span_off[d + 1] - B.span_off[d] - 1);
                const uint64_t prev_end = (uint64_t)B.start[s - 1] + B.len[s - 1];
                if (prev_end == 0) continue;
                bad.start[s] = 0;
                bad.len[s] = (uint32_t)(prev_end - 1);
                check_refused(bad, round);
            }
            if (B.span_off[d + 1] > B.span_off[d]) {
                Batch bad = B;
                bad.start[B.span_off[d + 1] - 1] = (uint32_t)L;
                bad.len[B.span_off[d + 1] - 1] = 1;
                check_refused(bad, round);
                break;
            }
        }
        if (B.s0) {                                                                                   // span_off[n_docs] < span_off[0]
            Batch bad = B;
            bad.span_off.back() = B.s0 - 1;
            check_refused(bad, round);
        }
    }
    if (fails) {
        std::fprintf(stderr, "excerpt_check: %d differences\n", fails);
        return 1;
    }
    std::printf("excerpt_check: %llu rounds, walk and brute force agree\n", (unsigned long long)rounds);
    return 0;
}
