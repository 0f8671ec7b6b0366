// select_check.cpp -- the select kernels' logic (csrc/gft_select_piece.hpp, run on the host by select_docs_host) against a
// byte-by-byte reference under the address and undefined-behaviour sanitizers: a stand-alone program, CPU only.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I. tools/select_check.cpp \
//       gofindthem_amd/csrc/select_host.cpp -o build/select_check
//   build/select_check 300
//
// Every input and output lies in a heap block of exactly its size: the text block holds blob[doc_off[0], doc_off[n]) and nothing
// else, the rows n * W words, the mask W words, the output cap_bytes bytes behind the `shift` bytes that put it on every residue
// of the 16-byte grid, the offsets cap_docs + 1 entries, the indices cap_docs.  A read outside the documents -- the host walk
// promises none -- or a store past a cap is then an error of the sanitizer; the bytes in front of a shifted output are checked
// by hand.  Batches: the fixed forms of tests/select_docs.py (built from the walk's own chunk, trip and tile sizes), then N seeded
// random ones; every one under the three modes, with full caps, count only, and caps that cut a document and the lists.
// Exit code 0: walk and reference agree everywhere.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "gofindthem_amd/csrc/gft_select.hpp"

using namespace gft;

namespace {

struct Batch {
    std::vector<uint8_t> text;           // the documents' bytes alone
    std::vector<uint64_t> off;           // [n + 1], off[0] = lead
    std::vector<uint32_t> rows;          // [n][W], tail bits ones
    std::vector<uint32_t> want;          // [W], tail bits ones
    bool want_null = false;
    std::vector<uint8_t> also;           // [n] or empty
    uint32_t n_cols = 0;
};

struct Result {
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> off, idx;
};

bool bit(const uint32_t* w, uint32_t j) { return w[j >> 5] >> (j & 31) & 1; }

// the contract of include/gft.h, one column and one byte at a time
Result reference(const Batch& B, uint32_t mode) {
    Result R;
    R.off.push_back(0);
    const uint64_t n = B.off.size() - 1;
    const uint32_t W = (B.n_cols + 31) / 32;
    for (uint64_t d = 0; d < n; d++) {
        bool any = false, all = true;
        for (uint32_t j = 0; j < B.n_cols; j++) {
            if (!B.want_null && !bit(B.want.data(), j)) continue;
            if (bit(B.rows.data() + d * W, j)) any = true; else all = false;
        }
        bool s = mode == GFT_SELECT_ANY ? any : mode == GFT_SELECT_ALL ? all : !any;
        if (!B.also.empty() && B.also[d]) s = true;
        if (!s) continue;
        for (uint64_t p = B.off[d]; p < B.off[d + 1]; p++) R.bytes.push_back(B.text[p - B.off[0]]);
        R.off.push_back(R.bytes.size());
        R.idx.push_back(d);
    }
    return R;
}

template <class T>
std::unique_ptr<T[]> exact(const std::vector<T>& v) {
    std::unique_ptr<T[]> p(new T[v.size() ? v.size() : 1]);
    if (!v.empty()) memcpy(p.get(), v.data(), v.size() * sizeof(T));
    return p;
}

int failures = 0;
uint64_t runs = 0;

void check(const std::string& name, const Batch& B) {
    const uint64_t n = B.off.size() - 1;
    auto text = exact(B.text);
    auto off = exact(B.off);
    auto rows = exact(B.rows);
    auto want = exact(B.want);
    auto also = exact(B.also);
    const uint8_t* blob = text.get() - B.off[0];                  // (only [off[0], off[n]) of it exists)
    for (uint32_t mode = 0; mode < 3; mode++) {
        const Result want_r = reference(B, mode);
        const uint64_t total = want_r.bytes.size(), m = want_r.idx.size();
        const uint64_t mid = m ? want_r.off[m / 2] + (want_r.off[m / 2 + 1] - want_r.off[m / 2]) / 2 : 0;
        const uint64_t caps[6][2] = {{total, m}, {0, 0}, {total ? total - 1 : 0, m ? m - 1 : 0}, {mid, 1}, {1, 0}, {total, m / 2}};
        for (uint32_t ci = 0; ci < 6; ci++) {
            const uint64_t cb = std::min(caps[ci][0], total + 3), cd = caps[ci][1];
            const uint32_t shift = (uint32_t)((runs * 7 + ci) % 16);
            std::unique_ptr<uint8_t[]> out(new uint8_t[shift + cb]);
            memset(out.get(), 0xA5, shift + cb);
            std::unique_ptr<uint64_t[]> oo(new uint64_t[cd + 1]), di(new uint64_t[cd]);
            for (uint64_t i = 0; i <= cd; i++) oo[i] = ~0ull;
            for (uint64_t i = 0; i < cd; i++) di[i] = ~0ull;
            uint64_t gm = ~0ull, gt = ~0ull;
            const bool count_only = ci == 1;
            const int rc = select_docs_host(blob, off.get(), n, B.n_cols ? rows.get() : nullptr, B.n_cols, B.want_null ? nullptr : want.get(), mode,
                                            B.also.empty() ? nullptr : also.get(), count_only ? nullptr : out.get() + shift, cb,
                                            count_only ? nullptr : oo.get(), count_only ? nullptr : di.get(), cd, &gm, &gt);
            runs++;
            bool ok = rc == GFT_OK && gm == m && gt == total;
            const uint64_t wb = std::min(total, cb), wd = std::min(m, cd);
            if (ok && !count_only) {
                for (uint64_t i = 0; ok && i < shift; i++) ok = out[i] == 0xA5;
                ok = ok && (!wb || !memcmp(out.get() + shift, want_r.bytes.data(), wb));
                for (uint64_t i = wb; ok && i < cb; i++) ok = out[shift + i] == 0xA5;
                for (uint64_t i = 0; ok && i <= cd; i++) ok = oo[i] == (i <= m ? want_r.off[i] : ~0ull);
                for (uint64_t i = 0; ok && i < cd; i++) ok = di[i] == (i < wd ? want_r.idx[i] : ~0ull);
            }
            if (!ok) {
                fprintf(stderr, "MISMATCH %s mode %u caps %llu %llu shift %u: rc %d m %llu (want %llu) total %llu (want %llu)\n", name.c_str(), mode,
                        (unsigned long long)cb, (unsigned long long)cd, shift, rc, (unsigned long long)gm, (unsigned long long)m,
                        (unsigned long long)gt, (unsigned long long)total);
                failures++;
            }
        }
    }
}

// a batch of documents of these lengths; density: the chance of a bit in a row; every tail bit is one
Batch make(std::mt19937_64& rng, const std::vector<uint64_t>& lengths, uint32_t n_cols, double density, int want_kind, bool with_also, uint64_t lead) {
    Batch B;
    B.n_cols = n_cols;
    const uint64_t n = lengths.size();
    const uint32_t W = (n_cols + 31) / 32;
    B.off.push_back(lead);
    for (uint64_t l : lengths) B.off.push_back(B.off.back() + l);
    B.text.resize(B.off.back() - lead);
    for (auto& b : B.text) b = (uint8_t)rng();
    B.rows.assign(n * W, 0);
    B.want.assign(W, 0);
    const uint64_t thr = (uint64_t)(density * 1000000.0);
    for (uint64_t d = 0; d < n; d++)
        for (uint32_t j = 0; j < n_cols; j++)
            if (rng() % 1000000 < thr) B.rows[d * W + (j >> 5)] |= 1u << (j & 31);
    B.want_null = want_kind == 0;                                  // 0: NULL, 1: empty, 2: a few columns, 3: a quarter of them
    if (want_kind >= 2)
        for (uint32_t j = 0; j < n_cols; j++)
            if (rng() % (want_kind == 2 ? n_cols : 4) == 0) B.want[j >> 5] |= 1u << (j & 31);
    if (n_cols & 31) {
        const uint32_t tail = ~0u << (n_cols & 31);
        for (uint64_t d = 0; d < n; d++) B.rows[d * W + W - 1] |= tail;
        B.want[W - 1] |= tail;
    }
    if (with_also) {
        B.also.assign(n, 0);
        for (auto& a : B.also) a = rng() % 50 == 0 ? (uint8_t)(1 + rng() % 255) : 0;
    }
    return B;
}

}  // namespace

int main(int argc, char** argv) {
    const uint64_t n_random = argc > 1 ? strtoull(argv[1], nullptr, 10) : 200;
    const uint64_t C = kSelChunk, TRIP = kSelTrip, TILE = kSelTile;
    std::mt19937_64 rng(20240707);
    const std::vector<uint64_t> edge = {0, 1, C - 1, C, C + 1, TRIP - 1, TRIP, TRIP + 1, TILE - 1, TILE + 1, 3 * TILE + 5};
    std::vector<uint64_t> twice = edge;
    twice.insert(twice.end(), edge.begin(), edge.end());
    std::vector<uint64_t> empties = {5, 1};
    empties.insert(empties.end(), 40, 0);
    empties.push_back(1); empties.push_back(9);
    std::vector<uint64_t> many_empties = {9, C};                    // more empty documents than a window holds: the search fallback
    many_empties.insert(many_empties.end(), 300, 0);
    many_empties.push_back(C); many_empties.push_back(9);
    std::vector<uint64_t> trip_empties = {TRIP};
    trip_empties.insert(trip_empties.end(), 300, 0);
    trip_empties.push_back(1); trip_empties.push_back(40);
    std::vector<uint64_t> stretch(3, 100);
    stretch.insert(stretch.end(), 5, 2 * TILE + 7);
    stretch.insert(stretch.end(), 300, 50);
    stretch.insert(stretch.end(), 3, 100);
    std::vector<uint64_t> mixed;
    for (uint64_t i = 0; i < 200; i++) mixed.push_back(i % 4);
    const uint32_t cols[] = {0, 1, 31, 32, 33, 70, 2048, 2081};
    for (uint32_t n_cols : cols)
        for (int want_kind = 0; want_kind < 4; want_kind++) {
            const std::string tag = " (" + std::to_string(n_cols) + " columns, mask " + std::to_string(want_kind) + ")";
            check("edge lengths" + tag, make(rng, twice, n_cols, 0.05, want_kind, false, 7));
            check("40 empty documents" + tag, make(rng, empties, n_cols, 0.3, want_kind, want_kind == 3, 0));
            check("300 empty documents" + tag, make(rng, many_empties, n_cols, 0.3, want_kind, false, 0));
            check("300 empty documents at the start of a trip" + tag, make(rng, trip_empties, n_cols, 0.3, want_kind, want_kind == 2, 5));
            check("200 one-byte documents" + tag, make(rng, std::vector<uint64_t>(200, 1), n_cols, 0.2, want_kind, false, 3));
            check("documents of 0 to 3 bytes" + tag, make(rng, mixed, n_cols, 0.1, want_kind, true, 0));
        }
    check("a long unselected stretch", make(rng, stretch, 40, 0.002, 0, true, 1));
    check("one document", make(rng, {TRIP + 5}, 3, 0.5, 0, false, 0));
    check("no documents", make(rng, {}, 40, 0.5, 0, false, 0));
    for (uint64_t r = 0; r < n_random; r++) {
        const uint64_t n = 1 + rng() % (r % 10 == 0 ? 5000 : 300);
        const double density = r % 3 == 0 ? 0.005 : r % 3 == 1 ? 0.1 : 0.9;
        const uint32_t n_cols = r % 7 == 0 ? 2081 : (uint32_t)(rng() % 100);
        std::vector<uint64_t> lengths(n);
        for (auto& l : lengths) l = rng() % 5 ? rng() % 40 : rng() % 3000;
        check("random " + std::to_string(r), make(rng, lengths, n_cols, density / (n_cols ? n_cols : 1) * 4, (int)(rng() % 4), rng() % 3 == 0, rng() % 20));
    }
    if (failures) { fprintf(stderr, "%d mismatches\n", failures); return 1; }
    printf("select_check: all cases agree (%llu runs of the walk)\n", (unsigned long long)runs);
    return 0;
}
