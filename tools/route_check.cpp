// route_check.cpp -- the route kernels' logic (csrc/gft_route_piece.hpp and the select's copy walk, run on the host by
// route_docs_host) against a naive reference under the address and undefined-behaviour sanitizers: a stand-alone program, CPU only.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I. tools/route_check.cpp \
//       gofindthem_amd/csrc/route_host.cpp gofindthem_amd/csrc/select_host.cpp -o build/route_check
//   build/route_check 300
//
// Every input and output lies in a heap block of exactly its size: the text block holds blob[doc_off[0], doc_off[n]) and nothing
// else, the rows n * W words, the masks K * W words, the output cap_bytes bytes behind the `shift` bytes that put it on every
// residue of the 16-byte grid, the offsets cap_docs + 1 entries, the indices cap_docs, the bucket arrays B + 1 entries.  A read
// outside the documents or a store past a cap is then an error of the sanitizer; the bytes in front of a shifted output are
// checked by hand.  Batches: N seeded random ones of 0 to 400 documents, 0 to 64 masks and rows of 0 to 2 100 columns, every one
// under both modes, with and without the rest bucket and `also`, with full caps, count only, and caps that cut a document and the
// lists.  Exit code 0: walk and reference agree everywhere.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "gofindthem_amd/csrc/gft_route.hpp"

using namespace gft;

namespace {

struct Batch {
    std::vector<uint8_t> text;           // the documents' bytes alone
    std::vector<uint64_t> off;           // [n + 1], off[0] = lead
    std::vector<uint32_t> rows;          // [n][W], tail bits ones
    std::vector<uint32_t> masks;         // [K][W], tail bits ones
    std::vector<uint8_t> also;           // [n]
    uint32_t n_cols = 0, K = 0;
};

struct Result {
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> off, idx, bucket_doc, bucket_byte;
};

bool bit(const uint32_t* w, uint32_t j) { return w[j >> 5] >> (j & 31) & 1; }

// the contract of include/gft.h, one bucket, one column and one byte at a time
Result reference(const Batch& B, uint32_t mode, bool rest, bool with_also) {
    Result R;
    R.off.push_back(0);
    const uint64_t n = B.off.size() - 1;
    const uint32_t W = (B.n_cols + 31) / 32, nb = B.K + (rest ? 1 : 0);
    for (uint32_t b = 0; b < nb; b++) {
        R.bucket_doc.push_back(R.idx.size());
        R.bucket_byte.push_back(R.bytes.size());
        for (uint64_t d = 0; d < n; d++) {
            int first = -1;
            bool mine = false;
            for (uint32_t k = 0; k < B.K; k++) {
                bool hit = false;
                for (uint32_t j = 0; j < B.n_cols && !hit; j++) hit = bit(B.masks.data() + (size_t)k * W, j) && bit(B.rows.data() + d * W, j);
                if (hit && first < 0) first = (int)k;
                if (hit && k == b) mine = true;
            }
            if (mode == GFT_ROUTE_FIRST) mine = first == (int)b;
            if (b == B.K) mine = first < 0;
            if (with_also && B.also[d]) mine = b == B.K;
            if (!mine) continue;
            for (uint64_t p = B.off[d]; p < B.off[d + 1]; p++) R.bytes.push_back(B.text[p - B.off[0]]);
            R.off.push_back(R.bytes.size());
            R.idx.push_back(d);
        }
    }
    R.bucket_doc.push_back(R.idx.size());
    R.bucket_byte.push_back(R.bytes.size());
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

void check(uint64_t seed, const Batch& B) {
    const uint64_t n = B.off.size() - 1;
    auto text = exact(B.text);
    auto off = exact(B.off);
    auto rows = exact(B.rows);
    auto masks = exact(B.masks);
    auto also = exact(B.also);
    const uint8_t* blob = text.get() - B.off[0];                  // (only [off[0], off[n]) of it exists)
    for (uint32_t form = 0; form < 6; form++) {
        const uint32_t mode = form & 1;
        const bool rest = form >= 2, with_also = form >= 4;
        if (rest && B.K == GFT_ROUTE_MAX_BUCKETS) continue;
        const uint32_t nb = B.K + (rest ? 1 : 0);
        const Result want = reference(B, mode, rest, with_also);
        const uint64_t total = want.bytes.size(), m = want.idx.size();
        const uint64_t mid = m ? want.off[m / 2] + (want.off[m / 2 + 1] - want.off[m / 2]) / 2 : 0;
        const uint64_t caps[6][2] = {{total, m}, {0, 0}, {total ? total - 1 : 0, m ? m - 1 : 0}, {mid, 1}, {1, 0}, {total, m / 2}};
        for (uint32_t ci = 0; ci < 6; ci++) {
            const uint64_t cb = std::min(caps[ci][0], total + 3), cd = caps[ci][1];
            const uint32_t shift = (uint32_t)((runs * 7 + ci) % 16);
            std::unique_ptr<uint8_t[]> out(new uint8_t[shift + cb]);
            memset(out.get(), 0xA5, shift + cb);
            std::unique_ptr<uint64_t[]> oo(new uint64_t[cd + 1]), di(new uint64_t[cd]), bd(new uint64_t[nb + 1]), bb(new uint64_t[nb + 1]);
            for (uint64_t i = 0; i <= cd; i++) oo[i] = ~0ull;
            for (uint64_t i = 0; i < cd; i++) di[i] = ~0ull;
            for (uint32_t i = 0; i <= nb; i++) bd[i] = bb[i] = ~0ull;
            const bool count_only = ci == 1;
            const int rc = route_docs_host(blob, off.get(), n, B.n_cols ? rows.get() : nullptr, B.n_cols, B.K && B.n_cols ? masks.get() : nullptr, B.K, mode,
                                           rest ? GFT_ROUTE_REST : 0, with_also ? also.get() : nullptr, count_only ? nullptr : out.get() + shift, cb,
                                           count_only ? nullptr : oo.get(), count_only ? nullptr : di.get(), cd, bd.get(), bb.get());
            runs++;
            bool ok = rc == GFT_OK;
            for (uint32_t i = 0; ok && i <= nb; i++) ok = bd[i] == want.bucket_doc[i] && bb[i] == want.bucket_byte[i];
            const uint64_t wb = std::min(total, cb), wd = std::min(m, cd);
            if (ok && !count_only) {
                for (uint64_t i = 0; ok && i < shift; i++) ok = out[i] == 0xA5;
                ok = ok && (!wb || !memcmp(out.get() + shift, want.bytes.data(), wb));
                for (uint64_t i = wb; ok && i < cb; i++) ok = out[shift + i] == 0xA5;
                for (uint64_t i = 0; ok && i <= cd; i++) ok = oo[i] == (i <= m ? want.off[i] : ~0ull);
                for (uint64_t i = 0; ok && i < cd; i++) ok = di[i] == (i < wd ? want.idx[i] : ~0ull);
            }
            if (!ok) {
                fprintf(stderr, "MISMATCH seed %llu: %llu documents, %u masks, %u columns, mode %u rest %d also %d caps %llu %llu shift %u: rc %d\n",
                        (unsigned long long)seed, (unsigned long long)n, B.K, B.n_cols, mode, (int)rest, (int)with_also, (unsigned long long)cb,
                        (unsigned long long)cd, shift, rc);
                failures++;
            }
        }
    }
}

Batch make(std::mt19937_64& rng) {
    static const uint32_t kCols[] = {0, 1, 31, 32, 33, 40, 64, 65, 257, 2048, 2080};
    static const uint32_t kMasks[] = {0, 1, 2, 3, 7, 20, 63, 64};
    Batch B;
    B.n_cols = kCols[rng() % 11];
    B.K = kMasks[rng() % 8];
    const uint64_t n = rng() % 5 == 0 ? rng() % 3 : rng() % 400, lead = rng() % 9;
    const uint32_t W = (B.n_cols + 31) / 32;
    B.off.push_back(lead);
    for (uint64_t d = 0; d < n; d++) B.off.push_back(B.off.back() + (rng() % 10 == 0 ? rng() % 6000 : rng() % 40));
    B.text.resize(B.off.back() - lead);
    for (auto& b : B.text) b = (uint8_t)rng();
    B.rows.assign(n * W, 0);
    B.masks.assign((size_t)B.K * W, 0);
    static const uint64_t kRowThr[] = {2000, 50000, 500000};
    const uint64_t row_thr = kRowThr[rng() % 3], mask_thr = B.n_cols > 100 ? 3000 : 100000;
    for (uint64_t d = 0; d < n; d++)
        for (uint32_t j = 0; j < B.n_cols; j++)
            if (rng() % 1000000 < row_thr) B.rows[d * W + (j >> 5)] |= 1u << (j & 31);
    for (uint32_t k = 0; k < B.K; k++)
        for (uint32_t j = 0; j < B.n_cols; j++)
            if (rng() % 1000000 < mask_thr || j + 1 == B.n_cols - k % 2) B.masks[(size_t)k * W + (j >> 5)] |= 1u << (j & 31);
    if (B.n_cols & 31) {                                              // the tail bits: ones everywhere
        const uint32_t tail = ~0u << (B.n_cols & 31);
        for (uint64_t d = 0; d < n; d++) B.rows[d * W + W - 1] |= tail;
        for (uint32_t k = 0; k < B.K; k++) B.masks[(size_t)k * W + W - 1] |= tail;
    }
    B.also.assign(n, 0);
    for (auto& a : B.also) a = rng() % 20 == 0 ? (uint8_t)(1 + rng() % 255) : 0;
    return B;
}

}  // namespace

int main(int argc, char** argv) {
    const uint64_t n_batches = argc > 1 ? strtoull(argv[1], nullptr, 10) : 100;
    for (uint64_t seed = 1; seed <= n_batches; seed++) {
        std::mt19937_64 rng(seed * 2654435761ull);
        check(seed, make(rng));
    }
    if (failures) {
        fprintf(stderr, "route_check: %d mismatches in %llu runs of the walk\n", failures, (unsigned long long)runs);
        return 1;
    }
    printf("route_check: all cases agree (%llu runs of the walk)\n", (unsigned long long)runs);
    return 0;
}
