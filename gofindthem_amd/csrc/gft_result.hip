// gft_result.hip -- rule rows of a batch -> the result document as text, the contract of rules_json.hpp on the device,
// gfx950 / wave64.
//
//   rows [n_docs][RW] (RW = ceil(R / 32)), hole_len [n_docs] (nullable), the fragment table of R entries and its blob  ->
//   out_off [n_docs + 1] u64, text [total] u8 = '[' D0 ',' D1 ... ']', Dd = {"rules":{"name":["expr",..],..}}
//
//   k_result<false>  cnt[d] = len(d) + 1 (the separator behind the document); a hole: hole_len[d] + 1, its row not loaded
//   (k_scan_partials / k_scan_spine / k_scan_final of gft_kernels.hip: cnt -> scan [n_docs + 1])
//   k_result<true>   out_off[d] = scan[d] + 1; the frame and the separators; every set bit's fragments copied to their offsets
//
// Both passes walk a row the same way, a wave a document: the lanes load 64 consecutive words, then every pair of words that
// holds a bit is taken as one 64-bit group, a lane a bit.  A lane's bit i is the first true expression of its rule when the set
// bit before it in the row -- a lower lane's, or the last of an earlier group, carried in `prev` -- lies below rule_first[i]:
// rules of any length and rules across word borders need nothing else.  Its cost is
//      first of its rule:  ("]," when a rule came before) + name fragment + expression fragment
//      otherwise:          "," + expression fragment
// and the fill pass places it at the exclusive prefix of the costs inside the group plus the bytes of the groups before.  Every
// lane copies its own fragments with a plain loop over the bytes, which the compiler widens to 16-byte loads and stores in its
// body: nothing is read behind a fragment, destinations have any alignment.
//
// Every store is below min(cap, the document's own end); a hole gets its separator and nothing else.  Bits at and above R in the
// last word are masked.  No shared memory, no atomics.  Memory bound: two reads of the rows plus the text.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gft_result.hpp"

namespace gft {

namespace {

constexpr uint32_t kResultBlock = 256;      // 4 waves
constexpr uint32_t kResultHead = 10;        // {"rules":{

struct TextOut {
    uint8_t* out;
    uint64_t limit;                         // min(cap, where the document's stores end)
    __device__ __forceinline__ void put(uint64_t at, uint8_t c) const { if (at < limit) out[at] = c; }
    // (the table and the text never overlap: the loads of a few bytes may be in flight together)
    __device__ __forceinline__ void copy(uint64_t at, const uint8_t* __restrict__ src, uint32_t len) const {
        if (at >= limit) return;
        const uint32_t n = (uint32_t)std::min<uint64_t>(len, limit - at);
        uint8_t* __restrict__ dst = out + at;
#pragma unroll 8
        for (uint32_t k = 0; k < n; k++) dst[k] = src[k];
    }
};

template <bool FILL>
__global__ void __launch_bounds__(kResultBlock) k_result(const ResultParams P) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * kResultBlock + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * kResultBlock) >> 6;
    if (FILL && !P.n_docs) {                // "[]"
        if (wave == 0 && lane == 0) {
            P.out_off[0] = 1;
            const TextOut T{P.out, P.cap};
            T.put(0, '[');
            T.put(1, ']');
        }
        return;
    }
    const uint32_t tail = (P.R & 31u) ? (1u << (P.R & 31u)) - 1 : 0xFFFFFFFFu;
    for (uint64_t d = wave; d < P.n_docs; d += n_waves) {
        const uint64_t hole = P.hole_len ? P.hole_len[d] : 0;        // (the same in every lane)
        uint64_t base = 0, end = 0;
        if (FILL) {
            base = P.scan[d] + 1;
            end = P.scan[d + 1] + 1;        // out_off[d + 1]: the separator is the byte before it
            if (lane == 0) {
                P.out_off[d] = base;
                const TextOut T{P.out, P.cap};
                if (d == 0) T.put(0, '[');
                if (d + 1 == P.n_docs) { P.out_off[d + 1] = end; T.put(end - 1, ']'); }
                else T.put(end - 1, ',');
            }
        }
        if (hole) {
            if (!FILL && lane == 0) {
                if (hole >= 0xFFFFFFFFull) { P.flags[0] = 1; P.cnt[d] = 1; }
                else P.cnt[d] = (uint32_t)hole + 1;
            }
            continue;
        }
        // the document's stores end before its separator, whatever the table says
        const TextOut T{P.out, FILL ? std::min(P.cap, end - 1) : 0};
        const uint32_t* row = P.rows + d * P.RW;
        int32_t prev = -1;                  // the last set bit of the groups before (the same in every lane)
        uint64_t at = base + kResultHead;   // fill: where the next group's bytes begin
        uint64_t acc = 0;                   // count: this lane's bytes
        for (uint32_t k = 0; k < P.RW; k += 64) {
            const uint32_t j = k + lane;
            const uint32_t w = j < P.RW ? row[j] & (j + 1 == P.RW ? tail : 0xFFFFFFFFu) : 0u;
            uint64_t nz = __ballot(w != 0);
            while (nz) {                    // (uniform: a pair of words with a bit, lowest first)
                const uint32_t c = (uint32_t)__builtin_ctzll(nz) >> 1;
                nz &= ~(3ull << (2 * c));
                const uint64_t m = (uint64_t)(uint32_t)__shfl((int)w, (int)(2 * c), 64) |
                                   (uint64_t)(uint32_t)__shfl((int)w, (int)(2 * c + 1), 64) << 32;
                const uint32_t bit0 = (k + 2 * c) * 32u;
                const uint64_t below = m & ((1ull << lane) - 1);
                const int32_t p = below ? (int32_t)(bit0 + 63u - (uint32_t)__builtin_clzll(below)) : prev;
                const bool set = m >> lane & 1ull;
                const uint32_t i = bit0 + lane;
                bool first = false;
                uint32_t name_len = 0, expr_len = 0;
                uint64_t cost = 0;
                if (set) {
                    first = p < (int32_t)P.rule_first[i];
                    expr_len = P.expr_len[i];
                    if (first) name_len = P.name_len[i];
                    cost = first ? (uint64_t)name_len + expr_len + (p >= 0 ? 2 : 0) : (uint64_t)expr_len + 1;
                }
                if (!FILL) {
                    acc += cost;
                } else {
                    uint64_t v = cost;
#pragma unroll
                    for (uint32_t s = 1; s < 64; s <<= 1) {
                        const uint64_t o = __shfl_up(v, s, 64);
                        if (lane >= s) v += o;
                    }
                    if (set) {
                        uint64_t pos = at + (v - cost);
                        if (first) {
                            if (p >= 0) { T.put(pos, ']'); T.put(pos + 1, ','); pos += 2; }
                            T.copy(pos, P.blob + P.name_off[i], name_len);
                            pos += name_len;
                        } else {
                            T.put(pos++, ',');
                        }
                        T.copy(pos, P.blob + P.expr_off[i], expr_len);
                    }
                    at += __shfl(v, 63, 64);
                }
                prev = (int32_t)(bit0 + 63u - (uint32_t)__builtin_clzll(m));
            }
        }
        if (!FILL) {
#pragma unroll
            for (uint32_t s = 1; s < 64; s <<= 1) acc += __shfl_xor(acc, (int)s, 64);
            // (the table's limit keeps this below 2^32: make_rule_fragments)
            if (lane == 0) P.cnt[d] = (uint32_t)(12 + acc + (prev >= 0 ? 1 : 0) + 1);
        } else if (lane == 0) {
            const TextOut H{P.out, T.limit};
            const char* head = "{\"rules\":{";
            for (uint32_t k = 0; k < kResultHead; k++) H.put(base + k, (uint8_t)head[k]);
            if (prev >= 0) H.put(at++, ']');
            H.put(at, '}');
            H.put(at + 1, '}');
        }
    }
}

unsigned result_grid(uint64_t n_docs, unsigned n_cus) {
    const uint64_t blocks = (n_docs + kResultBlock / 64 - 1) / (kResultBlock / 64);
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(blocks, (uint64_t)std::max(n_cus, 1u) * 8));   // 32 waves per CU
}

}  // namespace

hipError_t launch_result_count(const ResultParams& P, unsigned n_cus, hipStream_t st) {
    if (!P.n_docs) return hipSuccess;
    k_result<false><<<dim3(result_grid(P.n_docs, n_cus)), dim3(kResultBlock), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_result_fill(const ResultParams& P, unsigned n_cus, hipStream_t st) {
    k_result<true><<<dim3(result_grid(P.n_docs, n_cus)), dim3(kResultBlock), 0, st>>>(P);
    return hipGetLastError();
}

}  // namespace gft
