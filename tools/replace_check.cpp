// replace_check.cpp -- the replace kernels' logic (csrc/gft_replace_piece.hpp and the excerpt's run passes, run on the host by
// replace_spans_host) against an independent splice written here, under the address and undefined-behaviour sanitizers: a
// stand-alone program, CPU only.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I. tools/replace_check.cpp \
//       gofindthem_amd/csrc/replace_host.cpp gofindthem_amd/csrc/excerpt_host.cpp -o build/replace_check
//   build/replace_check 300
//
// Every input and output lies in a heap block of exactly its size -- the text of doc_off[n] bytes with no slack, the span arrays,
// the keys, the key map, the table, the output of cap bytes, the per-run arrays of cap_runs entries --, so a read outside them or a
// store past a cap is an error of the sanitizer.  N seeded random rounds, each: a random batch (empty documents, documents without
// spans, zero-length spans, spans that nest, repeat and touch, ends ascending, lead bytes in front of the first document), a
// random table of replacements of 0 .. GFT_REPLACE_MAX bytes with empty ones among them, keys NULL, keys that are ids, or keys
// through a key map; the output at a random residue of the 16-byte grid; every few rounds more spans than a tile, and once more
// than a carry trip's.  Every round draws a span base s0, 0 among the values: span_off[0] = s0, the span arrays are blocks of
// exactly s0 + n entries and the first s0 spans and keys are poison.  The brute force paints, per document, a grid of whole and
// half positions with the smallest id that reaches each point -- touching spans share a point, a gap of one byte leaves one
// unpainted --, reads the runs off the painted stretches, takes the smallest id of a stretch and splices byte by byte.  The walk
// runs under exact caps, count only, and caps that cut; then one span's end is put in front of its neighbour's, one span past its
// document's end and one key out of range, which must be refused with every output untouched.
// Exit code 0: walk and brute force agree everywhere.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "gofindthem_amd/csrc/gft_replace.hpp"

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
    std::vector<uint8_t> text, rep_bytes;
    std::vector<uint64_t> doc_off, span_off, rep_off;
    std::vector<uint32_t> start, len, key, key_rep;
    int mode = 0;                  // 0: no keys; 1: the key is the id; 2: through key_rep
    uint64_t s0 = 0;               // span_off[0]: the entries [0, s0) of start / len / key are poison
    uint32_t id_of(uint64_t s) const { return mode == 0 ? 0 : mode == 1 ? key[s] : key_rep[key[s]]; }
};

constexpr uint32_t kPoison = 0xFFFFFFFFu, kUntouched = 0xA5A5A5A5u;
constexpr uint64_t kUntouched64 = 0xA5A5A5A5A5A5A5A5ull;

struct Result {
    std::vector<uint8_t> out;
    std::vector<uint64_t> out_off, doc_run_off;
    std::vector<uint32_t> run_new, run_len, run_rep;
};

// the contract, by brute force
Result brute(const Batch& B) {
    Result R;
    const uint64_t n_docs = B.doc_off.size() - 1;
    R.out_off.push_back(0);
    R.doc_run_off.push_back(0);
    for (uint64_t d = 0; d < n_docs; d++) {
        const uint8_t* doc = B.text.data() + B.doc_off[d];
        const uint64_t L = B.doc_off[d + 1] - B.doc_off[d], doc_at = R.out.size();
        std::vector<uint32_t> grid(2 * L + 1, kPoison);             // point 2p: position p; point 2p + 1: inside byte p; the smallest id
        for (uint64_t s = B.span_off[d]; s < B.span_off[d + 1]; s++)
            for (uint64_t g = 2ull * B.start[s]; g <= 2ull * (B.start[s] + B.len[s]); g++) grid[g] = std::min(grid[g], B.id_of(s));
        for (uint64_t g = 0; g <= 2 * L;) {
            if (grid[g] == kPoison) {
                if (g & 1) R.out.push_back(doc[g / 2]);               // (a byte outside every run)
                g++;
                continue;
            }
            uint64_t h = g;
            uint32_t id = kPoison;
            while (h <= 2 * L && grid[h] != kPoison) id = std::min(id, grid[h++]);
            const uint64_t a = B.rep_off[id], b = B.rep_off[id + 1];
            R.run_new.push_back((uint32_t)(R.out.size() - doc_at));
            R.run_len.push_back((uint32_t)(b - a));
            R.run_rep.push_back(id);
            R.out.insert(R.out.end(), B.rep_bytes.begin() + a, B.rep_bytes.begin() + b);
            g = h;
        }
        R.out_off.push_back(R.out.size());
        R.doc_run_off.push_back(R.run_new.size());
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
    B.mode = (int)rnd(3);
    const uint32_t n_reps = 1 + (uint32_t)rnd(6), n_keys = 1 + (uint32_t)rnd(9);
    static const uint32_t lens[] = {0, 0, 0, 1, 2, 5, 15, 16, 17, 40, GFT_REPLACE_MAX};
    B.rep_off.push_back(0);
    for (uint32_t k = 0; k < n_reps; k++) {
        const uint32_t n = lens[rnd(11)];
        for (uint32_t i = 0; i < n; i++) B.rep_bytes.push_back((uint8_t)(1 + rnd(255)));
        B.rep_off.push_back(B.rep_bytes.size());
    }
    if (B.mode == 2)
        for (uint32_t k = 0; k < n_keys; k++) B.key_rep.push_back((uint32_t)rnd(n_reps));
    B.start.assign(B.s0, kPoison);
    B.len.assign(B.s0, kPoison);
    B.key.assign(B.s0, kPoison);
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
        for (auto& s : sp) {
            B.start.push_back((uint32_t)s.second);
            B.len.push_back((uint32_t)(s.first - s.second));
            B.key.push_back((uint32_t)rnd(B.mode == 2 ? n_keys : n_reps));
        }
        B.doc_off.push_back(B.text.size());
        B.span_off.push_back(B.start.size());
    }
    return B;
}

int fails = 0;
void expect(bool ok, const char* what, uint64_t round) {
    if (ok) return;
    fprintf(stderr, "round %llu: %s\n", (unsigned long long)round, what);
    fails++;
}

// the walk into heap blocks of exactly the sizes given; shift: the output's first byte that far into its block
int walk(const Batch& B, uint64_t cap, uint64_t cap_runs, uint32_t shift, Result& R, uint64_t& runs, uint64_t& total, uint8_t pat) {
    const uint64_t n_docs = B.doc_off.size() - 1;
    auto text = exact(B.text);
    auto off = exact(B.doc_off);
    auto so = exact(B.span_off);
    auto st = exact(B.start);
    auto ln = exact(B.len);
    auto ky = exact(B.key);
    auto kr = exact(B.key_rep);
    auto rb = exact(B.rep_bytes);
    auto ro = exact(B.rep_off);
    std::unique_ptr<uint8_t[]> out(new uint8_t[cap + shift]);      // (ends with the cap: a store behind it is the sanitizer's error)
    memset(out.get(), pat, cap + shift);
    R.out_off.assign(n_docs + 1, kUntouched64);
    R.doc_run_off.assign(n_docs + 1, kUntouched64);
    R.run_new.assign(cap_runs, kUntouched);
    R.run_len.assign(cap_runs, kUntouched);
    R.run_rep.assign(cap_runs, kUntouched);
    auto oo = exact(R.out_off);
    auto dro = exact(R.doc_run_off);
    auto rn = exact(R.run_new);
    auto rl = exact(R.run_len);
    auto rr = exact(R.run_rep);
    const bool none = B.start.empty();
    const int rc = replace_spans_host(text.get(), off.get(), n_docs, so.get(), none ? nullptr : st.get(), none ? nullptr : ln.get(),
                                      B.mode == 0 || none ? nullptr : ky.get(), B.mode == 2 ? kr.get() : nullptr, (uint32_t)B.key_rep.size(),
                                      B.rep_bytes.empty() ? nullptr : rb.get(), ro.get(), (uint32_t)B.rep_off.size() - 1, 0,
                                      cap ? out.get() + shift : nullptr, cap, oo.get(), dro.get(), cap_runs ? rn.get() : nullptr,
                                      cap_runs ? rl.get() : nullptr, cap_runs ? rr.get() : nullptr, cap_runs, &runs, &total);
    for (uint32_t i = 0; i < shift; i++)
        if (out[i] != pat) return -100;                             // (a store in front of the output)
    R.out.assign(out.get() + shift, out.get() + shift + cap);
    for (uint64_t d = 0; d <= n_docs; d++) { R.out_off[d] = oo[d]; R.doc_run_off[d] = dro[d]; }
    for (uint64_t r = 0; r < cap_runs; r++) { R.run_new[r] = rn[r]; R.run_len[r] = rl[r]; R.run_rep[r] = rr[r]; }
    return rc;
}

bool untouched(const Result& X) {
    return std::all_of(X.out.begin(), X.out.end(), [](uint8_t v) { return v == 0xA5; }) &&
           std::all_of(X.out_off.begin(), X.out_off.end(), [](uint64_t v) { return v == kUntouched64; }) &&
           std::all_of(X.doc_run_off.begin(), X.doc_run_off.end(), [](uint64_t v) { return v == kUntouched64; }) &&
           std::all_of(X.run_new.begin(), X.run_new.end(), [](uint32_t v) { return v == kUntouched; }) &&
           std::all_of(X.run_len.begin(), X.run_len.end(), [](uint32_t v) { return v == kUntouched; }) &&
           std::all_of(X.run_rep.begin(), X.run_rep.end(), [](uint32_t v) { return v == kUntouched; });
}

void one_round(uint64_t round, uint64_t want_spans) {
    const Batch B = random_batch(want_spans);
    const Result W = brute(B);
    const uint64_t total = W.out.size(), m = W.run_new.size();
    Result R;
    uint64_t runs = 0, bytes = 0;
    const uint32_t shift = (uint32_t)rnd(16);
    // exact caps
    expect(walk(B, total, m, shift, R, runs, bytes, 0xA5) == GFT_OK, "exact caps: refused", round);
    expect(runs == m && bytes == total, "exact caps: counts", round);
    expect(R.out == W.out, "exact caps: text", round);
    expect(R.out_off == W.out_off && R.doc_run_off == W.doc_run_off, "exact caps: offsets", round);
    expect(R.run_new == W.run_new && R.run_len == W.run_len && R.run_rep == W.run_rep, "exact caps: run arrays", round);
    // count only
    expect(walk(B, 0, 0, 0, R, runs, bytes, 0xA5) == GFT_OK && runs == m && bytes == total, "count only", round);
    expect(R.out_off == W.out_off && R.doc_run_off == W.doc_run_off, "count only: offsets", round);
    // caps that cut
    for (int i = 0; i < 3 && total; i++) {
        const uint64_t cap = rnd(total), cr = rnd(m + 1);
        const int rc = walk(B, cap, cr, (uint32_t)rnd(16), R, runs, bytes, 0x5A);
        expect(rc == GFT_OK && runs == m && bytes == total, "cut caps: counts", round);
        expect(std::equal(R.out.begin(), R.out.end(), W.out.begin()), "cut caps: text", round);
        expect(R.out_off == W.out_off && R.doc_run_off == W.doc_run_off, "cut caps: offsets", round);
        expect(std::equal(R.run_new.begin(), R.run_new.end(), W.run_new.begin()) && std::equal(R.run_len.begin(), R.run_len.end(), W.run_len.begin()) &&
                   std::equal(R.run_rep.begin(), R.run_rep.end(), W.run_rep.begin()),
               "cut caps: run arrays", round);
    }
    // the refusals: nothing is written
    for (uint64_t d = 0; d + 1 < B.doc_off.size(); d++) {
        const uint64_t a = B.span_off[d], b = B.span_off[d + 1], L = B.doc_off[d + 1] - B.doc_off[d];
        if (b - a < 2) continue;
        Result X;
        Batch C = B;
        C.start[b - 1] = 0; C.len[b - 1] = 0;                        // its end in front of its neighbour's ...
        if ((uint64_t)C.start[b - 2] + C.len[b - 2] != 0)
            expect(walk(C, total, m, shift, X, runs, bytes, 0xA5) == GFT_E_INVALID && runs == 0 && bytes == 0 && untouched(X), "order: not refused", round);
        C = B;
        C.len[b - 1] = (uint32_t)(L - C.start[b - 1] + 1);           // ... one byte past its document's end
        expect(walk(C, total, m, shift, X, runs, bytes, 0xA5) == GFT_E_INVALID && runs == 0 && bytes == 0 && untouched(X), "past the end: not refused", round);
        if (B.mode) {                                               // ... and a key out of range
            C = B;
            C.key[b - 1] = B.mode == 2 ? (uint32_t)B.key_rep.size() : (uint32_t)B.rep_off.size() - 1;
            expect(walk(C, total, m, shift, X, runs, bytes, 0xA5) == GFT_E_INVALID && runs == 0 && bytes == 0 && untouched(X), "key: not refused", round);
        }
        break;
    }
    if (B.s0 && B.doc_off.size() > 1) {                              // span_off[n_docs] < span_off[0]
        Batch C = B;
        C.span_off.back() = B.s0 - 1;
        Result X;
        expect(walk(C, total, m, shift, X, runs, bytes, 0xA5) == GFT_E_INVALID && runs == 0 && bytes == 0 && untouched(X), "offsets: not refused", round);
    }
}

}  // namespace

int main(int argc, char** argv) {
    const uint64_t rounds = argc > 1 ? strtoull(argv[1], nullptr, 10) : 300;
    rng.seed(20261020);
    for (uint64_t r = 0; r < rounds && fails < 10; r++) one_round(r, r % 25 == 7 ? kExcTile + rnd(3 * kExcTile) : 0);
    if (fails < 10) one_round(rounds, (uint64_t)kExcTile * kExcCarryTiles + 5);
    printf("replace_check: %llu rounds, %d failures\n", (unsigned long long)rounds + 1, fails);
    return fails ? 1 : 0;
}
