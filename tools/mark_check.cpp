// mark_check.cpp -- the highlight kernels' logic (csrc/gft_mark_piece.hpp and the excerpt's run passes, run on the host by
// mark_spans_host) against an independent splice written here, under the address and undefined-behaviour sanitizers: a stand-alone
// program, CPU only.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I. tools/mark_check.cpp \
//       gofindthem_amd/csrc/mark_host.cpp gofindthem_amd/csrc/excerpt_host.cpp -o build/mark_check
//   build/mark_check 300
//
// Every input and output lies in a heap block of exactly its size -- the text of doc_off[n] bytes with no slack, the span arrays,
// the markers, the output of cap bytes --, so a read outside them or a store past the cap is an error of the sanitizer.  N seeded
// random rounds, each: a random batch (empty documents, documents without spans, zero-length spans, spans that nest, repeat and
// touch, ends ascending, lead bytes in front of the first document), random markers of 0 .. GFT_MARK_MAX bytes, the output at a
// random residue of the 16-byte grid; every few rounds more spans than a tile, and once more than a carry trip's.  Every round
// draws a span base s0, 0 among the values: span_off[0] = s0, the span arrays and span_new are blocks of exactly s0 + n entries,
// the first s0 spans are poison, and the brute force is indexed the same way.  The brute force
// paints, per document, a grid of whole and half positions -- touching spans share a point, a gap of one byte leaves one
// unpainted --, reads the runs off the painted stretches and splices byte by byte.  The walk runs under an exact cap, count
// only, and caps that cut; then one span's end is put in front of its neighbour's and one span past its document's end, which must
// be refused with every output untouched.
// Exit code 0: walk and brute force agree everywhere.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "gofindthem_amd/csrc/gft_mark.hpp"

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
    std::vector<uint8_t> text, open, close;
    std::vector<uint64_t> doc_off, span_off;
    std::vector<uint32_t> start, len;
    uint64_t s0 = 0;               // span_off[0]: the entries [0, s0) of start / len are poison
};

constexpr uint32_t kPoison = 0xFFFFFFFFu, kUntouched = 0xA5A5A5A5u;

struct Result {
    std::vector<uint8_t> out;
    std::vector<uint64_t> out_off, doc_run_off;
    std::vector<uint32_t> span_new;
};

// the contract, by brute force
Result brute(const Batch& B) {
    Result R;
    const uint64_t n_docs = B.doc_off.size() - 1;
    R.out_off.push_back(0);
    R.doc_run_off.push_back(0);
    R.span_new.assign(B.start.size(), kUntouched);                 // (the entries below s0 are never written)
    uint64_t runs = 0;
    for (uint64_t d = 0; d < n_docs; d++) {
        const uint8_t* doc = B.text.data() + B.doc_off[d];
        const uint64_t L = B.doc_off[d + 1] - B.doc_off[d];
        std::vector<uint8_t> grid(2 * L + 1, 0);                    // point 2p: position p; point 2p + 1: inside byte p
        for (uint64_t s = B.span_off[d]; s < B.span_off[d + 1]; s++)
            for (uint64_t g = 2ull * B.start[s]; g <= 2ull * (B.start[s] + B.len[s]); g++) grid[g] = 1;
        std::vector<uint32_t> run_at(2 * L + 1, 0);                 // the run's index in the document, per painted point
        uint32_t r = 0;
        for (uint64_t g = 0; g <= 2 * L; g++) {
            if (!grid[g]) continue;
            if (g && grid[g - 1]) { run_at[g] = run_at[g - 1]; continue; }
            run_at[g] = r++;
        }
        for (uint64_t s = B.span_off[d]; s < B.span_off[d + 1]; s++) {
            const uint32_t k = run_at[2ull * B.start[s]];
            R.span_new[s] = (uint32_t)(B.start[s] + (k + 1) * B.open.size() + k * B.close.size());
        }
        for (uint64_t p = 0; p <= L; p++) {
            const bool here = grid[2 * p], before = p && grid[2 * p - 1], after = p < L && grid[2 * p + 1];
            if (here && before && !after) R.out.insert(R.out.end(), B.close.begin(), B.close.end());
            if (here && !before) R.out.insert(R.out.end(), B.open.begin(), B.open.end());
            if (here && !before && !after) R.out.insert(R.out.end(), B.close.begin(), B.close.end());
            if (p < L) R.out.push_back(doc[p]);
        }
        runs += r;
        R.out_off.push_back(R.out.size());
        R.doc_run_off.push_back(runs);
    }
    return R;
}

Batch random_batch(uint64_t want_spans) {
    Batch B;
    const uint64_t n_docs = want_spans ? 3 + rnd(3) : rnd(7);
    const uint64_t lead = rnd(20);
    B.text.assign(lead, 0xEE);
    B.doc_off.push_back(lead);
    static const uint64_t base[] = {0, 0, 1, 2, kExcTile - 1, kExcTile, kExcTile + 1, 3 * kExcTile + 7};
    B.s0 = rnd(9) < 8 ? base[rnd(8)] : rnd(1000);
    B.start.assign(B.s0, kPoison);
    B.len.assign(B.s0, kPoison);
    B.span_off.push_back(B.s0);
    for (uint64_t d = 0; d < n_docs; d++) {
        const uint64_t L = want_spans ? want_spans + rnd(50) : (rnd(4) ? rnd(150) : 0);
        for (uint64_t i = 0; i < L; i++) B.text.push_back((uint8_t)(1 + rnd(255)));
        std::vector<std::pair<uint64_t, uint64_t>> sp;             // (end, start)
        const uint64_t n = want_spans ? want_spans / n_docs + 1 : (rnd(3) ? rnd(10) : 0);
        for (uint64_t i = 0; i < n; i++) {
            const uint64_t a = rnd(L + 1), ln = std::min<uint64_t>(L - a, rnd(4) ? rnd(9) : 0);
            sp.push_back({a + ln, a});
        }
        std::sort(sp.begin(), sp.end());
        for (auto& s : sp) { B.start.push_back((uint32_t)s.second); B.len.push_back((uint32_t)(s.first - s.second)); }
        B.doc_off.push_back(B.text.size());
        B.span_off.push_back(B.start.size());
    }
    static const uint32_t lens[] = {0, 1, 2, 4, 5, 15, 16, 17, 40, GFT_MARK_MAX};
    B.open.resize(lens[rnd(10)]);
    B.close.resize(lens[rnd(10)]);
    for (auto& b : B.open) b = (uint8_t)(1 + rnd(255));
    for (auto& b : B.close) b = (uint8_t)(1 + rnd(255));
    return B;
}

int fails = 0;
void expect(bool ok, const char* what, uint64_t round) {
    if (ok) return;
    fprintf(stderr, "round %llu: %s\n", (unsigned long long)round, what);
    fails++;
}

// the walk into heap blocks of exactly the sizes given; shift: the output's first byte that far into its block
int walk(const Batch& B, uint64_t cap, uint32_t shift, Result& R, uint64_t& runs, uint64_t& total, uint8_t pat) {
    const uint64_t n_docs = B.doc_off.size() - 1;
    auto text = exact(B.text);
    auto off = exact(B.doc_off);
    auto so = exact(B.span_off);
    auto st = exact(B.start);
    auto ln = exact(B.len);
    auto open = exact(B.open);
    auto close = exact(B.close);
    std::unique_ptr<uint8_t[]> out(new uint8_t[cap + shift]);      // (ends with the cap: a store behind it is the sanitizer's error)
    memset(out.get(), pat, cap + shift);
    R.out_off.assign(n_docs + 1, 0xA5A5A5A5A5A5A5A5ull);
    R.doc_run_off.assign(n_docs + 1, 0xA5A5A5A5A5A5A5A5ull);
    R.span_new.assign(B.start.size(), kUntouched);
    auto oo = exact(R.out_off);
    auto dro = exact(R.doc_run_off);
    auto sn = exact(R.span_new);
    const int rc = mark_spans_host(text.get(), off.get(), n_docs, so.get(), B.start.empty() ? nullptr : st.get(), B.len.empty() ? nullptr : ln.get(),
                                   B.open.empty() ? nullptr : open.get(), (uint32_t)B.open.size(), B.close.empty() ? nullptr : close.get(),
                                   (uint32_t)B.close.size(), 0, cap ? out.get() + shift : nullptr, cap, oo.get(), B.start.empty() ? nullptr : sn.get(),
                                   dro.get(), &runs, &total);
    for (uint32_t i = 0; i < shift; i++)
        if (out[i] != pat) return -100;                             // (a store in front of the output)
    R.out.assign(out.get() + shift, out.get() + shift + cap);
    for (uint64_t d = 0; d <= n_docs; d++) { R.out_off[d] = oo[d]; R.doc_run_off[d] = dro[d]; }
    for (size_t s = 0; s < B.start.size(); s++) R.span_new[s] = sn[s];
    return rc;
}

void one_round(uint64_t round, uint64_t want_spans) {
    const Batch B = random_batch(want_spans);
    const Result W = brute(B);
    const uint64_t total = W.out.size();
    Result R;
    uint64_t runs = 0, bytes = 0;
    const uint32_t shift = (uint32_t)rnd(16);
    // an exact cap
    expect(walk(B, total, shift, R, runs, bytes, 0xA5) == GFT_OK, "exact cap: refused", round);
    expect(runs == W.doc_run_off.back() && bytes == total, "exact cap: counts", round);
    expect(R.out == W.out, "exact cap: text", round);
    expect(R.out_off == W.out_off && R.doc_run_off == W.doc_run_off && R.span_new == W.span_new, "exact cap: index arrays", round);
    // count only
    expect(walk(B, 0, 0, R, runs, bytes, 0xA5) == GFT_OK && runs == W.doc_run_off.back() && bytes == total, "count only", round);
    expect(R.out_off == W.out_off && R.span_new == W.span_new, "count only: index arrays", round);
    // caps that cut
    for (int i = 0; i < 3 && total; i++) {
        const uint64_t cap = rnd(total);
        const int rc = walk(B, cap, (uint32_t)rnd(16), R, runs, bytes, 0x5A);
        expect(rc == GFT_OK && runs == W.doc_run_off.back() && bytes == total, "cut cap: counts", round);
        expect(std::equal(R.out.begin(), R.out.end(), W.out.begin()), "cut cap: text", round);
        expect(R.out_off == W.out_off && R.doc_run_off == W.doc_run_off && R.span_new == W.span_new, "cut cap: index arrays", round);
    }
    // the two refusals: nothing is written
    for (uint64_t d = 0; d + 1 < B.doc_off.size(); d++) {
        const uint64_t a = B.span_off[d], b = B.span_off[d + 1], L = B.doc_off[d + 1] - B.doc_off[d];
        if (b - a < 2) continue;
        Batch C = B;
        C.start[b - 1] = 0; C.len[b - 1] = 0;                        // its end in front of its neighbour's ...
        if ((uint64_t)C.start[b - 2] + C.len[b - 2] == 0) continue;
        Result X;
        expect(walk(C, total, shift, X, runs, bytes, 0xA5) == GFT_E_INVALID && runs == 0 && bytes == 0, "order: not refused", round);
        expect(std::all_of(X.out.begin(), X.out.end(), [](uint8_t v) { return v == 0xA5; }), "order: text written", round);
        expect(std::all_of(X.out_off.begin(), X.out_off.end(), [](uint64_t v) { return v == 0xA5A5A5A5A5A5A5A5ull; }), "order: offsets written", round);
        expect(std::all_of(X.span_new.begin(), X.span_new.end(), [](uint32_t v) { return v == 0xA5A5A5A5u; }), "order: span_new written", round);
        C = B;
        C.len[b - 1] = (uint32_t)(L - C.start[b - 1] + 1);           // ... and one byte past its document's end
        expect(walk(C, total, shift, X, runs, bytes, 0xA5) == GFT_E_INVALID && runs == 0 && bytes == 0, "past the end: not refused", round);
        expect(std::all_of(X.out.begin(), X.out.end(), [](uint8_t v) { return v == 0xA5; }), "past the end: text written", round);
        expect(std::all_of(X.doc_run_off.begin(), X.doc_run_off.end(), [](uint64_t v) { return v == 0xA5A5A5A5A5A5A5A5ull; }), "past the end: offsets written", round);
        break;
    }
    if (B.s0 && B.doc_off.size() > 1) {                              // span_off[n_docs] < span_off[0]
        Batch C = B;
        C.span_off.back() = B.s0 - 1;
        Result X;
        expect(walk(C, total, shift, X, runs, bytes, 0xA5) == GFT_E_INVALID && runs == 0 && bytes == 0, "offsets: not refused", round);
        expect(std::all_of(X.out.begin(), X.out.end(), [](uint8_t v) { return v == 0xA5; }), "offsets: text written", round);
        expect(std::all_of(X.span_new.begin(), X.span_new.end(), [](uint32_t v) { return v == kUntouched; }), "offsets: span_new written", round);
    }
}

}  // namespace

int main(int argc, char** argv) {
    const uint64_t rounds = argc > 1 ? strtoull(argv[1], nullptr, 10) : 300;
    rng.seed(20261020);
    for (uint64_t r = 0; r < rounds && fails < 10; r++) one_round(r, r % 25 == 7 ? kExcTile + rnd(3 * kExcTile) : 0);
    if (fails < 10) one_round(rounds, (uint64_t)kExcTile * kExcCarryTiles + 5);
    printf("mark_check: %llu rounds, %d failures\n", (unsigned long long)rounds + 1, fails);
    return fails ? 1 : 0;
}
