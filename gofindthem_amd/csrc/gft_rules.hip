// gft_rules.hip -- the group finder's rule evaluation for records (rule_set.hpp), gfx950 / wave64.
//
//   hit rows [n_leaves][EW]  --k_leaf_tags-->  tag rows [n_leaves][TW]   (bit t: some expression of tag t is true)
//   tag rows + leaf_field + rec_off  --k_record_rules-->  rule bitmap [n_records][RW]
//
// k_record_rules is bit-sliced like the solver: a workgroup takes 64 records, a 64-bit word holds one answer per record.
//   phase 1  unit_word[u] in LDS, a thread per UNIT (tag, mask): bit i is set when a leaf of record i lies in a field of the
//            mask and carries the tag.  The block's leaves are one contiguous range; it is staged through LDS in chunks of
//            256 (field and record-in-block of every leaf), so records of uneven size cost what their leaves cost.  A thread
//            is the only writer of its words: no atomics.
//   phase 2  a thread per rule expression, 256 per trip: its postfix program over the 64-bit words, operand stack in LDS
//            (entry d of thread t at d * 256 + t: conflict free).
//   phase 3  the trip's 256 answers are transposed through LDS: a thread per (record, output word) gathers 32 bits and
//            stores the word.  Every word of the result is written exactly once, with plain stores.
// Both kernels also validate what they read: a field index outside the schema sets flags[0], record offsets that descend or
// leave [0, n_leaves] set flags[1] (plain stores of 1); such leaves / records are skipped, never dereferenced.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gft_rules.hpp"

namespace gft {

namespace {

constexpr uint32_t kLeafTagsBlock = 256;

__global__ void __launch_bounds__(kLeafTagsBlock) k_leaf_tags(const uint32_t* __restrict__ hit, uint32_t EW, uint32_t n_exprs,
                                                          const uint32_t* __restrict__ expr_tag, const uint32_t* __restrict__ leaf_field,
                                                          uint32_t n_fields, uint64_t n_leaves, uint32_t TW, uint32_t* __restrict__ tag_rows,
                                                          uint32_t* __restrict__ flags) {
    const uint64_t stride = (uint64_t)gridDim.x * kLeafTagsBlock;
    if (TW == 0) {                                  // a finder without expressions: nothing to fold, the fields are still checked
        for (uint64_t l = (uint64_t)blockIdx.x * kLeafTagsBlock + threadIdx.x; l < n_leaves; l += stride)
            if (leaf_field[l] >= n_fields) flags[0] = 1;
        return;
    }
    const uint64_t total = n_leaves * TW;
    for (uint64_t idx = (uint64_t)blockIdx.x * kLeafTagsBlock + threadIdx.x; idx < total; idx += stride) {
        const uint64_t l = idx / TW;
        const uint32_t tw = (uint32_t)(idx - l * TW);
        if (tw == 0 && leaf_field[l] >= n_fields) flags[0] = 1;
        const uint32_t* row = hit + l * EW;
        uint32_t acc = 0;
        for (uint32_t w = 0; w < EW; w++) {
            uint32_t bits = row[w];
            if (w + 1 == EW && (n_exprs & 31)) bits &= (1u << (n_exprs & 31)) - 1;     // garbage above n_exprs is ignored
            while (bits) {
                const uint32_t t = expr_tag[w * 32 + (uint32_t)__builtin_ctz(bits)];
                bits &= bits - 1;
                if ((t >> 5) == tw) acc |= 1u << (t & 31);
            }
        }
        tag_rows[idx] = acc;
    }
}

__global__ void __launch_bounds__(kRuleBlock) k_record_rules(const RulesParams P) {
    extern __shared__ __align__(16) uint8_t smem[];
    uint64_t* s_off = reinterpret_cast<uint64_t*>(smem);                     // [65]: offsets of the block's 64 records; [65]: the block is broken
    uint64_t* unit_word = s_off + 66;                                        // [n_units]
    uint64_t* res = unit_word + P.n_units;                                   // [256]
    uint64_t* stk = res + kRuleBlock;                                        // [max_depth][256]
    uint32_t* s_field = reinterpret_cast<uint32_t*>(stk + (size_t)P.max_depth * kRuleBlock);   // [256]
    uint32_t* s_rec = s_field + kRuleBlock;                                  // [256]

    const uint32_t tid = threadIdx.x;
    const uint64_t r0 = (uint64_t)blockIdx.x * 64;
    if (tid == 0) s_off[65] = 0;
    __syncthreads();
    if (tid <= 64) {
        const uint64_t r = r0 + tid < P.n_records ? r0 + tid : P.n_records;   // records past the batch are empty
        s_off[tid] = P.rec_off[r];
    }
    if (blockIdx.x == 0 && tid == 0 && P.rec_off[P.n_records] != P.n_leaves) P.flags[1] = 1;
    __syncthreads();
    if (tid < 64 && (s_off[tid] > s_off[tid + 1] || s_off[tid + 1] > P.n_leaves)) s_off[65] = 1;
    for (uint32_t u = tid; u < P.n_units; u += kRuleBlock) unit_word[u] = 0;
    __syncthreads();
    const bool bad = s_off[65] != 0;                                             // (uniform) a broken block has no leaves at all
    if (bad && tid == 0) P.flags[1] = 1;
    const uint64_t first = bad ? 0 : s_off[0], last = bad ? 0 : s_off[64];

    // ---- phase 1
    for (uint64_t base = first; base < last; base += kRuleBlock) {
        const uint32_t n = (uint32_t)(last - base < kRuleBlock ? last - base : kRuleBlock);
        if (tid < n) {
            const uint64_t l = base + tid;
            uint32_t lo = 0, hi = 64;                                        // the record i with s_off[i] <= l < s_off[i + 1]
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (s_off[mid] <= l) lo = mid; else hi = mid;
            }
            const uint32_t f = P.leaf_field[l];
            if (f >= P.n_fields) P.flags[0] = 1;
            s_field[tid] = f < P.n_fields ? f : 0xFFFFFFFFu;
            s_rec[tid] = lo;
        }
        __syncthreads();
        for (uint32_t u = tid; u < P.n_units; u += kRuleBlock) {
            const uint32_t tag = P.units[2 * u], m = P.units[2 * u + 1];
            if (tag == kRuleNoTag) continue;
            const uint32_t* mrow = P.masks + (size_t)m * P.FW;
            const uint32_t* trow = P.tag_rows + base * P.TW + (tag >> 5);
            uint64_t word = 0;
            for (uint32_t j = 0; j < n; j++) {
                const uint32_t f = s_field[j];
                if (f == 0xFFFFFFFFu) continue;
                const uint32_t in_mask = mrow[f >> 5] >> (f & 31) & 1u;
                const uint32_t has_tag = trow[(size_t)j * P.TW] >> (tag & 31) & 1u;
                word |= (uint64_t)(in_mask & has_tag) << s_rec[j];
            }
            unit_word[u] |= word;
        }
        __syncthreads();
    }
    __syncthreads();

    // ---- phases 2 and 3, 256 rule expressions per trip
    for (uint32_t k0 = 0; k0 < P.n_rules; k0 += kRuleBlock) {
        const uint32_t k = k0 + tid;
        uint64_t val = 0;
        if (k < P.n_rules) {
            uint32_t sp = 0;
            const uint32_t end = P.prog_off[k + 1];
            for (uint32_t i = P.prog_off[k]; i < end; i++) {
                const uint32_t w = P.prog[i];
                const uint32_t op = w >> 28;
                if (op == kRopUnit) {
                    stk[sp * kRuleBlock + tid] = unit_word[w & 0x0FFFFFFFu];
                    sp++;
                } else if (op == kRopNot) {
                    stk[(sp - 1) * kRuleBlock + tid] = ~stk[(sp - 1) * kRuleBlock + tid];
                } else {
                    sp--;
                    const uint64_t b = stk[sp * kRuleBlock + tid], a = stk[(sp - 1) * kRuleBlock + tid];
                    stk[(sp - 1) * kRuleBlock + tid] = op == kRopAnd ? (a & b) : (a | b);
                }
            }
            val = stk[tid];
        }
        res[tid] = val;                                                      // rules past n_rules answer zero
        __syncthreads();
        for (uint32_t item = tid; item < 64 * (kRuleBlock / 32); item += kRuleBlock) {
            const uint32_t i = item / (kRuleBlock / 32), w = item % (kRuleBlock / 32);
            uint32_t word = 0;
#pragma unroll 8
            for (uint32_t b = 0; b < 32; b++) word |= (uint32_t)(res[w * 32 + b] >> i & 1ull) << b;
            const uint32_t gw = k0 / 32 + w;
            if (r0 + i < P.n_records && gw < P.RW) P.out[(r0 + i) * P.RW + gw] = word;
        }
        __syncthreads();
    }
}

}  // namespace

size_t rules_lds_bytes(uint32_t n_units, uint32_t max_depth) {
    return (size_t)(66 + n_units + kRuleBlock + (size_t)max_depth * kRuleBlock) * 8 + 2 * kRuleBlock * 4;
}

hipError_t launch_leaf_tags(const uint32_t* d_hit, uint32_t n_exprs, const uint32_t* d_expr_tag, const uint32_t* d_leaf_field, uint32_t n_fields,
                            uint64_t n_leaves, uint32_t n_tags, uint32_t* d_tag_rows, uint32_t* d_flags, hipStream_t st) {
    const uint32_t TW = (n_tags + 31) / 32;
    if (!n_leaves) return hipSuccess;
    const uint64_t blocks = (n_leaves * (TW ? TW : 1) + kLeafTagsBlock - 1) / kLeafTagsBlock;
    k_leaf_tags<<<dim3((unsigned)std::min<uint64_t>(blocks, 1u << 20)), dim3(kLeafTagsBlock), 0, st>>>(
        d_hit, (n_exprs + 31) / 32, n_exprs, d_expr_tag, d_leaf_field, n_fields, n_leaves, TW, d_tag_rows, d_flags);
    return hipGetLastError();
}

hipError_t launch_record_rules(const RulesParams& P, size_t lds_max, hipStream_t st) {
    if (!P.n_records) return hipSuccess;            // (a set without rules still has its batch checked: no trip of phase 2)
    const uint64_t blocks = (P.n_records + 63) / 64;
    const size_t lds = rules_lds_bytes(P.n_units, P.max_depth);
    if (lds + 64 > lds_max || blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_record_rules), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    k_record_rules<<<dim3((unsigned)blocks), dim3(kRuleBlock), lds, st>>>(P);
    return hipGetLastError();
}

}  // namespace gft
