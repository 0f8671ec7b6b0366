// context_check.cpp -- the context kernels' logic (csrc/gft_context_piece.hpp, run on the host by context_docs_host) against a
// document-by-document brute force under the address and undefined-behaviour sanitizers: a stand-alone program, CPU only.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I. tools/context_check.cpp \
//       gofindthem_amd/csrc/context_host.cpp gofindthem_amd/csrc/select_host.cpp -o build/context_check
//   build/context_check 300
//
// Every input and output lies in a heap block of exactly its size: the text block holds blob[doc_off[0], doc_off[n]) and nothing
// else, the rows n * W words, the fences n bytes, the output cap_bytes bytes behind the `shift` bytes that put it on every residue
// of the 16-byte grid, the offsets cap_docs + 1 entries, the indices and kinds cap_docs, the groups cap_groups + 1.  A read outside
// the documents or a store past a cap is then an error of the sanitizer.  The brute force walks from every document towards its
// neighbours, one document at a time, until it meets a selected one, a fence or the end of its reach.  Batches: the shapes of
// tests/context_docs.py (document counts round a tile, the carry-block border, lone hits, reaches over empty tiles and over a
// carry block, 2^64 - 1, fences everywhere), then N seeded random ones; every one with full caps, count only and cut caps.
// Exit code 0: walk and brute force agree everywhere.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "gofindthem_amd/csrc/gft_context.hpp"

using namespace gft;

namespace {

struct Batch {
    std::vector<uint8_t> text;           // the documents' bytes alone
    std::vector<uint64_t> off;           // [n + 1], off[0] = lead
    std::vector<uint32_t> rows;          // [n][W], tail bits ones
    std::vector<uint8_t> also;           // [n] or empty
    std::vector<uint8_t> fence;          // [n] or empty
    uint32_t n_cols = 0;
    uint64_t before = 0, after = 0;
};

struct Result {
    std::vector<uint8_t> bytes, kind;
    std::vector<uint64_t> off, idx, groups;
    uint64_t hits = 0;
};

// the contract of include/gft.h, one document at a time (want: every column)
Result reference(const Batch& B, uint32_t mode) {
    Result R;
    R.off.push_back(0);
    const uint64_t n = B.off.size() - 1;
    const uint32_t W = (B.n_cols + 31) / 32;
    std::vector<uint8_t> sel(n, 0), keep(n, 0);
    for (uint64_t d = 0; d < n; d++) {
        bool any = false, all = true;
        for (uint32_t j = 0; j < B.n_cols; j++)
            if (B.rows[d * W + (j >> 5)] >> (j & 31) & 1) any = true; else all = false;
        bool s = mode == GFT_SELECT_ANY ? any : mode == GFT_SELECT_ALL ? all : !any;
        if (!B.also.empty() && B.also[d]) s = true;
        sel[d] = s;
    }
    auto fence_at = [&](uint64_t d) { return !B.fence.empty() && B.fence[d] != 0; };
    for (uint64_t d = 0; d < n; d++) {
        bool k = sel[d];
        // a selected h in front of d: d - h <= after, no fence in (h, d]
        for (uint64_t h = d, steps = 0; !k && h > 0 && steps < B.after && !fence_at(h); steps++) k = sel[--h];
        // ... behind d: h - d <= before, no fence in (d, h]
        for (uint64_t h = d, steps = 0; !k && h + 1 < n && steps < B.before && !fence_at(h + 1); steps++) k = sel[++h];
        keep[d] = k;
    }
    for (uint64_t d = 0; d < n; d++) {
        if (!keep[d]) continue;
        if (d == 0 || !keep[d - 1] || fence_at(d)) R.groups.push_back(R.idx.size());
        for (uint64_t p = B.off[d]; p < B.off[d + 1]; p++) R.bytes.push_back(B.text[p - B.off[0]]);
        R.off.push_back(R.bytes.size());
        R.idx.push_back(d);
        R.kind.push_back(sel[d]);
        R.hits += sel[d];
    }
    R.groups.push_back(R.idx.size());
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

void check(const std::string& name, const Batch& B, uint32_t mode) {
    const uint64_t n = B.off.size() - 1;
    auto text = exact(B.text);
    auto off = exact(B.off);
    auto rows = exact(B.rows);
    auto also = exact(B.also);
    auto fence = exact(B.fence);
    const uint8_t* blob = text.get() - B.off[0];                  // (only [off[0], off[n]) of it exists)
    const Result want = reference(B, mode);
    const uint64_t total = want.bytes.size(), m = want.idx.size(), g = want.groups.size() - 1;
    const uint64_t mid = m ? want.off[m / 2] + (want.off[m / 2 + 1] - want.off[m / 2]) / 2 : 0;
    const uint64_t caps[5][3] = {{total, m, g}, {0, 0, 0}, {total ? total - 1 : 0, m ? m - 1 : 0, g ? g - 1 : 0}, {mid, 1, g}, {total + 3, m / 2, 1}};
    for (uint32_t ci = 0; ci < 5; ci++) {
        const uint64_t cb = caps[ci][0], cd = caps[ci][1], cg = caps[ci][2];
        const uint32_t shift = (uint32_t)((runs * 7 + ci) % 16);
        std::unique_ptr<uint8_t[]> out(new uint8_t[shift + cb]), ki(new uint8_t[cd ? cd : 1]);
        memset(out.get(), 0xA5, shift + cb);
        memset(ki.get(), 0xA5, cd ? cd : 1);
        std::unique_ptr<uint64_t[]> oo(new uint64_t[cd + 1]), di(new uint64_t[cd ? cd : 1]), go(new uint64_t[cg + 1]);
        for (uint64_t i = 0; i <= cd; i++) oo[i] = ~0ull;
        for (uint64_t i = 0; i < cd; i++) di[i] = ~0ull;
        for (uint64_t i = 0; i <= cg; i++) go[i] = ~0ull;
        uint64_t gm = ~0ull, gh = ~0ull, gg = ~0ull, gt = ~0ull;
        const bool count_only = ci == 1;
        const int rc = context_docs_host(blob, off.get(), n, B.n_cols ? rows.get() : nullptr, B.n_cols, nullptr, mode, B.also.empty() ? nullptr : also.get(),
                                         B.before, B.after, B.fence.empty() ? nullptr : fence.get(), count_only ? nullptr : out.get() + shift, cb,
                                         count_only ? nullptr : oo.get(), count_only ? nullptr : di.get(), count_only ? nullptr : ki.get(), cd,
                                         count_only ? nullptr : go.get(), cg, &gm, &gh, &gg, &gt);
        runs++;
        bool ok = rc == GFT_OK && gm == m && gh == want.hits && gg == g && gt == total;
        const uint64_t wb = std::min(total, cb), wd = std::min(m, cd);
        if (ok && !count_only) {
            for (uint64_t i = 0; ok && i < shift; i++) ok = out[i] == 0xA5;
            ok = ok && (!wb || !memcmp(out.get() + shift, want.bytes.data(), wb));
            for (uint64_t i = wb; ok && i < cb; i++) ok = out[shift + i] == 0xA5;
            for (uint64_t i = 0; ok && i <= cd; i++) ok = oo[i] == (i <= m ? want.off[i] : ~0ull);
            for (uint64_t i = 0; ok && i < cd; i++) ok = di[i] == (i < wd ? want.idx[i] : ~0ull) && ki[i] == (i < wd ? want.kind[i] : 0xA5);
            for (uint64_t i = 0; ok && i <= cg; i++) ok = go[i] == (i <= g ? want.groups[i] : ~0ull);
        }
        if (!ok) {
            fprintf(stderr, "MISMATCH %s mode %u caps %llu %llu %llu shift %u: rc %d kept %llu (want %llu) hits %llu (%llu) groups %llu (%llu) total %llu (%llu)\n",
                    name.c_str(), mode, (unsigned long long)cb, (unsigned long long)cd, (unsigned long long)cg, shift, rc, (unsigned long long)gm,
                    (unsigned long long)m, (unsigned long long)gh, (unsigned long long)want.hits, (unsigned long long)gg, (unsigned long long)g,
                    (unsigned long long)gt, (unsigned long long)total);
            failures++;
        }
    }
}

// n documents of 0 to 40 bytes, the ones in `hits` selected under ANY (column 0 of n_cols; the other columns clear, tail bits ones)
Batch make(std::mt19937_64& rng, uint64_t n, const std::vector<uint64_t>& hits, uint64_t before, uint64_t after, const std::vector<uint64_t>& fences,
           uint32_t n_cols = 3, uint64_t lead = 0, bool null_fence = false) {
    Batch B;
    B.n_cols = n_cols; B.before = before; B.after = after;
    const uint32_t W = (n_cols + 31) / 32;
    B.off.push_back(lead);
    for (uint64_t d = 0; d < n; d++) B.off.push_back(B.off.back() + rng() % 41);
    B.text.resize(B.off.back() - lead);
    for (auto& b : B.text) b = (uint8_t)rng();
    B.rows.assign(n * W, 0);
    if (n_cols)
        for (uint64_t h : hits) B.rows[h * W] |= 1u;
    else {
        B.also.assign(n, 0);
        for (uint64_t h : hits) B.also[h] = (uint8_t)(1 + rng() % 255);
    }
    if (n_cols & 31)
        for (uint64_t d = 0; d < n; d++) B.rows[d * W + W - 1] |= ~0u << (n_cols & 31);
    if (!null_fence) {
        B.fence.assign(n, 0);
        for (uint64_t f : fences) B.fence[f] = (uint8_t)(1 + rng() % 255);
    }
    return B;
}

std::vector<uint64_t> some(std::mt19937_64& rng, uint64_t n, double density) {
    std::vector<uint64_t> v;
    for (uint64_t d = 0; d < n; d++)
        if (rng() % 1000000 < (uint64_t)(density * 1000000.0)) v.push_back(d);
    return v;
}

}  // namespace

int main(int argc, char** argv) {
    const uint64_t n_random = argc > 1 ? strtoull(argv[1], nullptr, 10) : 200;
    const uint64_t T = kCtxTile, B = (uint64_t)kCtxTile * kCtxCarry, MAX = ~0ull;
    std::mt19937_64 rng(20250909);
    for (uint64_t n : {(uint64_t)1, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1})
        for (uint32_t mode = 0; mode < 3; mode++) {
            const std::string tag = std::to_string(n) + " documents";
            check(tag, make(rng, n, some(rng, n, 0.08), 1, 2, {}), mode);
            check(tag + ", fences", make(rng, n, some(rng, n, 0.08), 3, 1, some(rng, n, 0.1), 33, 3), mode);
            check(tag + ", the last one hit", make(rng, n, {n - 1}, 2, 2, {}, 70), mode);
        }
    {
        const uint64_t n = B + T + 5;
        check("carry border, behind", make(rng, n, {B - 1}, 0, 3, {}), 0);
        check("carry border, in front", make(rng, n, {B}, 3, 0, {}), 0);
        check("carry border, either side", make(rng, n, {B - T + 3, B + T - 3}, T - 5, T - 5, {}), 0);
        check("carry border, over it behind", make(rng, n, {B - T - 1}, 0, T + 2, {}), 0);
        check("carry border, over it in front", make(rng, n, {B + T}, T + 1, 0, {}), 0);
        check("carry border, a fence on it", make(rng, n, {B - 2, B + 1}, 5, 5, {B}), 0);
        check("carry border, a fence behind it", make(rng, n, {B - 2}, 5, 5, {B + 1}), 0);
    }
    {
        const uint64_t n = 3 * T + 8;
        check("lone hit at 0", make(rng, n, {0}, 3, 3, {}), 0);
        check("lone hit at n - 1", make(rng, n, {n - 1}, 3, 3, {}), 0);
        check("lone hit, last lane, after 1", make(rng, n, {2 * T - 1}, 0, 1, {}), 0);
        check("lone hit, first lane, before 1", make(rng, n, {2 * T}, 1, 0, {}), 0);
        check("lone hit, last lane, before 1", make(rng, n, {2 * T - 1}, 1, 0, {}), 0);
        check("lone hit, first lane, after 1", make(rng, n, {2 * T}, 0, 1, {}), 0);
    }
    for (uint64_t k : {(uint64_t)1, (uint64_t)3}) {
        const uint64_t n = (k + 2) * T + 9;
        for (uint64_t r : {T * k - 1, T * k, T * k + 1}) {
            check("after over empty tiles", make(rng, n, {10}, 0, r, {}), 0);
            check("before over empty tiles", make(rng, n, {n - 11}, r, 0, {}), 0);
            check("both over empty tiles", make(rng, n, {T - 1, n - 1}, r, r, {}), 0);
        }
    }
    {
        const uint64_t n = 2 * B + 100;
        check("longer than a carry block, behind", make(rng, n, {5}, 0, B + 70, {}), 0);
        check("longer than a carry block, in front", make(rng, n, {n - 3}, B + 70, 0, {}), 0);
        check("longer than a carry block, fences", make(rng, n, {5, n - 3}, B + 70, B + 70, {B + 9, B + 11}), 0);
        check("no limit over two carry blocks", make(rng, n, {B + 1}, MAX, MAX, {}, 3, 0, true), 0);
    }
    check("before 2^64 - 1", make(rng, 300, {150}, MAX, 0, {40, 260}), 0);
    check("after 2^64 - 1", make(rng, 300, {150}, 0, MAX, {40, 260}), 0);
    check("both 2^64 - 1, no fence array", make(rng, 300, {150}, MAX, MAX, {}, 3, 0, true), 0);
    check("both 2^64 - 1, hits at either end", make(rng, 300, {0, 299}, MAX, MAX, {100, 200}), 0);
    check("nothing selected", make(rng, 130, {}, 2, 2, {5, 64}), 0);
    check("everything selected", make(rng, 130, {}, 2, 2, {}), 2);
    {
        std::vector<uint64_t> all;
        for (uint64_t d = 0; d < 2 * T + 20; d++) all.push_back(d);
        check("a fence on every document", make(rng, all.size(), {7, T, T + 1, all.size() - 1}, 4, 4, all), 0);
        check("everything selected, a fence on every document", make(rng, all.size(), all, 2, 2, all), 0);
    }
    for (uint64_t a : {(uint64_t)20, T - 3})
        for (uint64_t gap : {2, 3, 4}) check("two hits", make(rng, 2 * T + 3, {a, a + gap}, 1, 1, {}), 0);
    check("a fence at 0", make(rng, 148, {0, 3}, 5, 5, {0}), 0);
    check("a fence at the tile border", make(rng, 148, {T - 2, T + 2}, 5, 5, {T}), 0);
    check("a fence in the last lane", make(rng, 148, {T - 3, T + 1}, 5, 5, {T - 1}), 0);
    check("a fence right behind a hit", make(rng, 148, {30}, 3, 3, {31}), 0);
    check("a fence on the hit", make(rng, 148, {30}, 3, 3, {30}), 0);
    check("a fence on a hit among hits", make(rng, 148, {29, 30, 31}, 1, 1, {30}), 0);
    for (uint32_t n_cols : {0u, 20u, 70u, 65u * 32u})
        for (uint32_t mode = 0; mode < 3; mode++) check("row widths", make(rng, 150, some(rng, 150, 0.06), 2, 1, {70, 78}, n_cols, 7), mode);
    check("no documents", make(rng, 0, {}, 2, 2, {}), 0);
    const uint64_t reaches[] = {0, 1, 2, 5, 63, 64, 65, 700, MAX};
    for (uint64_t r = 0; r < n_random; r++) {
        const uint64_t n = 1 + rng() % 700;
        const double density = r % 3 == 0 ? 0.005 : r % 3 == 1 ? 0.05 : 0.3;
        const double fd = (r / 3) % 3 == 0 ? 0.0 : (r / 3) % 3 == 1 ? 0.02 : 0.3;
        Batch b = make(rng, n, some(rng, n, density), reaches[rng() % 9], reaches[rng() % 9], some(rng, n, fd), (uint32_t)(rng() % 80), rng() % 20,
                       (r / 3) % 3 == 0);
        if (r % 5 == 4 && b.also.empty()) {
            b.also.assign(n, 0);
            for (auto& a : b.also) a = rng() % 100 == 0;
        }
        check("random " + std::to_string(r), b, (uint32_t)(r % 3));
    }
    if (failures) { fprintf(stderr, "%d mismatches\n", failures); return 1; }
    printf("context_check: all cases agree (%llu runs of the walk)\n", (unsigned long long)runs);
    return 0;
}
