// gft_tagdoc.hip -- leaf hit rows of a record batch -> the tag result document as text, the contract of tags_json.hpp on the
// device, gfx950 / wave64.
//
//   hit rows [n_leaves][EW], leaf_field [n_leaves], rec_off [n_records + 1], hole_len [n_records] (nullable), the slot and field
//   tables and their blobs  ->  out_off [n_records + 1] u64, text [total] u8 = '[' D0 ',' D1 ... ']',
//   Dd = {"tags":{"tag":{"path":["expr",..],..},..}}
//
//   k_tag_slots      slot_rows[l][w]: a thread an output word, bit s the OR of the hit bits of slot s's expressions (a gather
//                    through the CSR of the slots' sources: no atomics); a leaf that does not contribute: zero, its row not read
//   k_tagdoc<false>  cnt[d] = len(d) + 1 (the separator behind the document); a hole: hole_len[d] + 1, its leaves not loaded
//   (k_scan_partials / k_scan_spine / k_scan_final of gft_kernels.hip: cnt -> scan [n_records + 1])
//   k_tagdoc<true>   out_off[d] = scan[d] + 1; the frame and the separators; every set slot bit's fragments copied to their offsets
//
// Both passes of k_tagdoc walk a record the same way, a wave a record.  The wave ranks the record's contributing leaves by
// field_rank in LDS -- a leaf's position is the number of contributing leaves with a smaller rank; equal ranks are "a field
// twice" -- and then walks the virtual word sequence (tag, leaf in rank order, word of the tag's range): the lanes load 64
// consecutive words of it, then the words that hold a bit are taken two at a time, a half wave a word, a lane a bit.  Tags
// begin at word borders, so all bits of a word share their tag and leaf, and what a bit costs depends on the set bit before it
// in its word or else on the (tag, leaf) of the non-zero word before -- the other half's, or the one carried from the round before:
//      a lower bit in the word, or the same tag and leaf before:  "," + expression fragment
//      the same tag, another leaf before:                         "]," + field fragment + expression fragment
//      another tag before:                                        "]}," + tag fragment + field fragment + expression fragment
//      nothing before:                                            tag fragment + field fragment + expression fragment
// The fill pass places a bit at the exclusive prefix of the costs inside the round plus the bytes of the rounds before.  Every
// lane copies its own fragments with a plain loop over the bytes (TextOut::copy, the form of gft_result.hip).
//
// Every store is below min(cap, the document's own end); a hole gets its separator and nothing else.  Lengths are counted in 64
// bits.  No atomics, no inline assembly.  Memory bound: the hit rows once, the slot rows written once and read twice, the text.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gft_tagdoc.hpp"
#include "gft_wave_dev.hpp"

namespace gft {

namespace {

constexpr uint32_t kTagDocBlock = 256;      // 4 waves
constexpr uint32_t kTagDocHead = 9;         // {"tags":{
constexpr uint32_t kNoRank = 0xFFFFFFFFu;
constexpr uint32_t kMaxLeaves = GFT_TAGS_JSON_MAX_LEAVES;

__global__ void __launch_bounds__(kTagDocBlock) k_tag_slots(const TagDocParams P) {
    const uint64_t n_words = P.n_leaves * P.SW;
    const uint64_t n_threads = (uint64_t)gridDim.x * kTagDocBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kTagDocBlock + threadIdx.x; i < n_words; i += n_threads) {
        const uint64_t leaf = i / P.SW;
        const uint32_t w = (uint32_t)(i - leaf * P.SW);
        const uint32_t f = P.leaf_field[leaf];
        uint32_t word = 0;
        if (f >= P.n_fields) {
            if (w == 0) P.flags[kTagDocFlagField] = 1;
        } else if (P.valid[f >> 5] >> (f & 31) & 1u) {
            const uint32_t* row = P.hits + leaf * P.EW;
            uint32_t k = P.src_off[w * 32u];
            for (uint32_t s = 0; s < 32; s++) {
                const uint32_t end = P.src_off[w * 32u + s + 1];
                uint32_t bit = 0;
                for (; k < end; k++) {
                    const uint32_t x = P.src_expr[k];
                    bit |= row[x >> 5] >> (x & 31) & 1u;
                }
                word |= bit << s;
            }
        }
        P.slot_rows[i] = word;
    }
}

struct TextOut {
    uint8_t* out;
    uint64_t limit;                         // min(cap, where the document's stores end)
    __device__ __forceinline__ void put(uint64_t at, uint8_t c) const { if (at < limit) out[at] = c; }
    // (the tables and the text never overlap: the loads of a few bytes may be in flight together)
    __device__ __forceinline__ void copy(uint64_t at, const uint8_t* __restrict__ src, uint32_t len) const {
        if (at >= limit) return;
        const uint32_t n = (uint32_t)std::min<uint64_t>(len, limit - at);
        uint8_t* __restrict__ dst = out + at;
#pragma unroll 8
        for (uint32_t k = 0; k < n; k++) dst[k] = src[k];
    }
};

template <bool FILL>
__global__ void __launch_bounds__(kTagDocBlock) k_tagdoc(const TagDocParams P) {
    __shared__ uint32_t s_rank[kTagDocBlock / 64][kMaxLeaves];   // a leaf's field rank, kNoRank: it does not contribute
    __shared__ uint32_t s_ord[kTagDocBlock / 64][kMaxLeaves];    // the contributing leaves in rank order
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t* rank = s_rank[threadIdx.x >> 6];
    uint32_t* ord = s_ord[threadIdx.x >> 6];
    const uint64_t wave = ((uint64_t)blockIdx.x * kTagDocBlock + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * kTagDocBlock) >> 6;
    if (FILL && !P.n_records) {             // "[]"
        if (wave == 0 && lane == 0) {
            P.out_off[0] = 1;
            const TextOut T{P.out, P.cap};
            T.put(0, '[');
            T.put(1, ']');
        }
        return;
    }
    for (uint64_t d = wave; d < P.n_records; d += n_waves) {
        const uint64_t hole = P.hole_len ? P.hole_len[d] : 0;        // (the same in every lane)
        const uint64_t o0 = P.rec_off[d], o1 = P.rec_off[d + 1];
        const bool offsets_ok = o0 <= o1 && o1 <= P.n_leaves;
        if (!FILL && lane == 0 && (!offsets_ok || (d + 1 == P.n_records && o1 != P.n_leaves))) P.flags[kTagDocFlagOffsets] = 1;
        uint64_t base = 0, end = 0;
        if (FILL) {
            base = P.scan[d] + 1;
            end = P.scan[d + 1] + 1;        // out_off[d + 1]: the separator is the byte before it
            if (lane == 0) {
                P.out_off[d] = base;
                const TextOut T{P.out, P.cap};
                if (d == 0) T.put(0, '[');
                if (d + 1 == P.n_records) { P.out_off[d + 1] = end; T.put(end - 1, ']'); }
                else T.put(end - 1, ',');
            }
        }
        if (hole) {
            if (!FILL && lane == 0) {
                if (hole >= 0xFFFFFFFFull) { P.flags[kTagDocFlagHole] = 1; P.cnt[d] = 1; }
                else P.cnt[d] = (uint32_t)hole + 1;
            }
            continue;
        }
        // ---- the record's contributing leaves in rank order (such offsets are never used as an index)
        bool refused = false;               // (the same in every lane)
        uint32_t L = 0;
        if (offsets_ok) {
            if (o1 - o0 > kMaxLeaves) {
                refused = true;
                if (!FILL && lane == 0) P.flags[kTagDocFlagLeaves] = 1;
            } else {
                L = (uint32_t)(o1 - o0);
            }
        }
        wave_lds_fence();                        // (the record before is done with the arrays)
        for (uint32_t i = lane; i < L; i += 64) {
            const uint32_t f = P.leaf_field[o0 + i];
            uint32_t r = kNoRank;
            if (f >= P.n_fields) { if (!FILL) P.flags[kTagDocFlagField] = 1; }
            else if (P.valid[f >> 5] >> (f & 31) & 1u) r = P.field_rank[f];
            rank[i] = r;
        }
        wave_lds_fence();
        uint32_t mine = 0;
        bool twice = false;
        for (uint32_t i = lane; i < L; i += 64) {
            const uint32_t r = rank[i];
            if (r == kNoRank) continue;
            uint32_t pos = 0;
            for (uint32_t j = 0; j < L; j++) {
                const uint32_t q = rank[j];
                pos += q < r;
                twice |= q == r && j != i;
            }
            ord[pos] = i;                   // (pos < L whatever the ranks)
            mine++;
        }
        if (__any(twice)) {
            refused = true;                 // (positions collide: ord is not a permutation and is not read)
            if (!FILL && lane == 0) P.flags[kTagDocFlagTwice] = 1;
        }
#pragma unroll
        for (uint32_t s = 1; s < 64; s <<= 1) mine += (uint32_t)__shfl_xor((int)mine, (int)s, 64);
        const uint32_t n_contrib = refused ? 0 : mine;
        wave_lds_fence();
        // ---- the walk.  The document's stores end before its separator, whatever the tables say
        const TextOut T{P.out, FILL ? std::min(P.cap, end - 1) : 0};
        int32_t prev_tag = -1, prev_pos = -1;   // of the last non-zero word of the rounds before (the same in every lane)
        uint64_t at = base + kTagDocHead;   // fill: where the next round's bytes begin
        uint64_t acc = 0;                   // count: this lane's bytes
        for (uint32_t t = 0; t < P.n_tags && n_contrib; t++) {
            const uint32_t tw = P.tag_words[t], w0 = P.tag_word[t];
            const uint64_t n = (uint64_t)n_contrib * tw;
            for (uint64_t k0 = 0; k0 < n; k0 += 64) {
                const uint64_t j = k0 + lane;
                uint32_t w = 0;
                if (j < n) {
                    const uint32_t p = tw == 1 ? (uint32_t)j : (uint32_t)(j / tw);
                    const uint32_t k = (uint32_t)(j - (uint64_t)p * tw);
                    w = P.slot_rows[(o0 + ord[p]) * P.SW + w0 + k];
                }
                uint64_t nz = __ballot(w != 0);
                while (nz) {                // (uniform: the next two words with a bit, a half wave each)
                    const uint32_t c0 = (uint32_t)__builtin_ctzll(nz);
                    nz &= nz - 1;
                    const bool two = nz != 0;
                    const uint32_t c1 = two ? (uint32_t)__builtin_ctzll(nz) : c0;
                    nz &= nz - 1;           // (0 stays 0)
                    const uint32_t p0 = tw == 1 ? (uint32_t)(k0 + c0) : (uint32_t)((k0 + c0) / tw);
                    const uint32_t p1 = tw == 1 ? (uint32_t)(k0 + c1) : (uint32_t)((k0 + c1) / tw);
                    const bool upper = lane >= 32;
                    const uint32_t c = upper ? c1 : c0, p = upper ? p1 : p0;
                    uint32_t m = (uint32_t)__shfl((int)w, (int)c, 64);
                    if (upper && !two) m = 0;
                    const uint32_t bit = lane & 31u;
                    const bool set = m >> bit & 1u;
                    // the set bit before: a lower one of the word, else the last of the non-zero word before
                    const bool lower = (m & ((1u << bit) - 1)) != 0;
                    const int32_t qt = upper ? (int32_t)t : prev_tag, qp = upper ? (int32_t)p0 : prev_pos;
                    uint32_t kind = 0;      // 0: "," + expression; 1: a new leaf; 2: a new tag
                    uint32_t expr_off = 0, expr_len = 0, field = 0, field_len = 0, tag_len = 0;
                    uint64_t cost = 0;
                    if (set) {
                        const uint32_t k = (uint32_t)(k0 + c - (uint64_t)p * tw);
                        const uint32_t s = (w0 + k) * 32u + bit;
                        expr_off = P.slot_off[s];
                        expr_len = P.slot_len[s];
                        if (!lower && !(qt == (int32_t)t && qp == (int32_t)p)) {
                            kind = qt == (int32_t)t ? 1 : 2;
                            field = P.leaf_field[o0 + ord[p]];
                            field_len = P.field_len[field];
                            if (kind == 2) tag_len = P.tag_len[t];
                        }
                        cost = kind == 0 ? (uint64_t)expr_len + 1
                             : kind == 1 ? (uint64_t)expr_len + field_len + 2
                                         : (uint64_t)expr_len + field_len + tag_len + (qt >= 0 ? 3 : 0);
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
                            if (kind == 0) {
                                T.put(pos++, ',');
                            } else {
                                if (kind == 1) { T.put(pos, ']'); T.put(pos + 1, ','); pos += 2; }
                                else {
                                    if (qt >= 0) { T.put(pos, ']'); T.put(pos + 1, '}'); T.put(pos + 2, ','); pos += 3; }
                                    T.copy(pos, P.slot_blob + P.tag_off[t], tag_len);
                                    pos += tag_len;
                                }
                                T.copy(pos, P.field_blob + P.field_off[field], field_len);
                                pos += field_len;
                            }
                            T.copy(pos, P.slot_blob + expr_off, expr_len);
                        }
                        at += __shfl(v, 63, 64);
                    }
                    prev_tag = (int32_t)t;
                    prev_pos = (int32_t)(two ? p1 : p0);
                }
            }
        }
        if (!FILL) {
#pragma unroll
            for (uint32_t s = 1; s < 64; s <<= 1) acc += __shfl_xor(acc, (int)s, 64);
            if (lane == 0) {
                const uint64_t len = kTagDocHead + acc + (prev_tag >= 0 ? 2 : 0) + 2;
                if (len + 1 > 0xFFFFFFFFull) { P.flags[kTagDocFlagLong] = 1; P.cnt[d] = 1; }
                else P.cnt[d] = refused ? 1u : (uint32_t)len + 1;
            }
        } else if (lane == 0 && !refused) {
            const TextOut H{P.out, T.limit};
            const char* head = "{\"tags\":{";
            for (uint32_t k = 0; k < kTagDocHead; k++) H.put(base + k, (uint8_t)head[k]);
            if (prev_tag >= 0) { H.put(at, ']'); H.put(at + 1, '}'); at += 2; }
            H.put(at, '}');
            H.put(at + 1, '}');
        }
    }
}

unsigned tagdoc_grid(uint64_t n_records, unsigned n_cus) {
    const uint64_t blocks = (n_records + kTagDocBlock / 64 - 1) / (kTagDocBlock / 64);
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(blocks, (uint64_t)std::max(n_cus, 1u) * 8));
}

}  // namespace

hipError_t launch_tag_slots(const TagDocParams& P, hipStream_t st) {
    const uint64_t n_words = P.n_leaves * P.SW;
    if (!n_words) return hipSuccess;
    const uint64_t blocks = std::min<uint64_t>((n_words + kTagDocBlock - 1) / kTagDocBlock, 1u << 20);
    k_tag_slots<<<dim3((unsigned)blocks), dim3(kTagDocBlock), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_tagdoc_count(const TagDocParams& P, unsigned n_cus, hipStream_t st) {
    if (!P.n_records) return hipSuccess;
    k_tagdoc<false><<<dim3(tagdoc_grid(P.n_records, n_cus)), dim3(kTagDocBlock), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_tagdoc_fill(const TagDocParams& P, unsigned n_cus, hipStream_t st) {
    k_tagdoc<true><<<dim3(tagdoc_grid(P.n_records, n_cus)), dim3(kTagDocBlock), 0, st>>>(P);
    return hipGetLastError();
}

}  // namespace gft
