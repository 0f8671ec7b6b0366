// gft_rank.hip -- a score per document (gft_score_docs_device), the k best documents of a score array (gft_top_docs_device) and the
// place pass of documents gathered by an index list (gft_gather_docs_device), gfx950 / wave64.
//
//   (off, term), weights  ->  score[d]          score  ->  top_idx, top_score          idx  ->  (len, c_src) for the select's copy
//
//   k_score_docs     the statistics' walk (gft_stats_piece.hpp) behind the statistics' check pass: a workgroup owns a range of whole
//                    documents (stats_cut) and walks it in steps; a lane an entry, the entry's document by a search in the step's
//                    offsets (LDS), its weight from LDS (from global memory above kRankWeightLdsTerms) added to the document's 64-bit
//                    sum in LDS; a document of kStatsLarge entries or more is summed in registers by the whole workgroup.  The
//                    distinct mode asks the step's set / the large path's bitset first (gft_stats_dev.hpp).  A document has one
//                    owner: its score goes out by a plain store.  The only global atomic is one maximum per wave into the control
//                    block
//   k_top_max        the largest score, for a caller that does not know it
//   k_top_hist       one digit of the radix select: LDS bins per workgroup over the keys that share the prefix, one atomic per
//                    workgroup and non-empty bin into the pass's row of the global table
//   k_top_pick       one wave: the digit that holds the rank still looked for, into the prefix; the rank inside it
//   k_top_count      per tile of kRankPlaceTile documents: scores above the threshold, scores equal to it
//   k_top_place      the same ballots again, behind the tiles' prefix sums: candidates into their slots
//   k_top_sort       one workgroup: the candidates through a bitonic network in LDS (rank_before), both arrays out
//   k_gather_place   a lane a list entry: the index checked against n_docs, the document's length and where it lies in the text
//
// No workgroup waits for another; every store is a vector store.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gft_rank.hpp"
#include "gft_stats_dev.hpp"
#include "gft_wave_dev.hpp"

namespace gft {

namespace {

typedef unsigned long long ull;

// the sum / the maximum of v over the wave, in every lane
__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
#pragma unroll
    for (int s = 32; s; s >>= 1) v += shuffle_xor64(v, s);
    return v;
}
__device__ __forceinline__ uint64_t wave_max64(uint64_t v) {
#pragma unroll
    for (int s = 32; s; s >>= 1) v = std::max(v, shuffle_xor64(v, s));
    return v;
}

__global__ void __launch_bounds__(kRankBlock) k_score_docs(const ScoreParams P) {
    __shared__ uint64_t s_set[kStatsSetSlots];                      // the step's set; the large path's bitset
    __shared__ uint64_t s_sum[kStatsStepDocs];                      // the step's documents' sums
    __shared__ uint32_t s_rel[kStatsStepDocs + 1];
    __shared__ uint32_t s_w[kRankWeightLdsTerms];
    __shared__ uint64_t s_red[kRankBlock / 64];
    if (P.ctl[kStatsCtlOffs] | P.ctl[kStatsCtlTerms]) return;       // (the same in every lane)
    const uint32_t tid = threadIdx.x;
    const bool w_lds = P.weights && rank_weights_in_lds(P.n_terms);
    for (uint32_t s = tid; s < kStatsSetSlots; s += kRankBlock) s_set[s] = 0;
    if (w_lds)
        for (uint32_t t = tid; t < P.n_terms; t += kRankBlock) s_w[t] = P.weights[t];
    __syncthreads();
    const uint64_t dlo = stats_cut(P.off, P.n_docs, blockIdx.x, P.grid), dhi = stats_cut(P.off, P.n_docs, blockIdx.x + 1u, P.grid);
    uint32_t* const bits = P.rows ? P.rows + (uint64_t)blockIdx.x * stats_bitset_words(P.n_terms) : reinterpret_cast<uint32_t*>(s_set);
    uint64_t top = 0;                                               // the largest score this lane stored
    for (uint64_t d = dlo; d < dhi;) {
        const uint64_t e0 = P.off[d];
        const uint32_t tries = dhi - d < kStatsStepDocs ? (uint32_t)(dhi - d) : kStatsStepDocs;
        for (uint32_t k = tid; k <= tries; k += kRankBlock) s_rel[k] = stats_rel(P.off[d + k], e0);
        for (uint32_t k = tid; k < tries; k += kRankBlock) s_sum[k] = 0;
        __syncthreads();
        const LdsRel rel{s_rel};
        const uint32_t nd = stats_step_docs(rel, tries);
        if (nd) {
            const uint32_t ne = s_rel[nd];
            uint32_t fst = 0, mine[kRankTrips];
#pragma unroll
            for (uint32_t j = 0; j < kRankTrips; j++) {
                const uint32_t i = j * kRankBlock + tid;
                mine[j] = 0;
                if (i >= ne) continue;
                const uint32_t t = P.term[e0 + i];
                const uint32_t dl = stats_find_doc(rel, nd, i);
                if (P.distinct) {
                    if (!stats_set_first(s_set, dl, t, mine[j])) continue;
                    fst |= 1u << j;
                }
                const uint32_t w = !P.weights ? 1u : w_lds ? s_w[t] : P.weights[t];
                if (w) atomicAdd(reinterpret_cast<ull*>(&s_sum[dl]), (ull)w);
            }
            __syncthreads();                                        // (every key is in the set before the first is taken out)
#pragma unroll
            for (uint32_t j = 0; j < kRankTrips; j++)
                if (fst >> j & 1) s_set[mine[j]] = 0;               // the set is empty again for the next step
            for (uint32_t k = tid; k < nd; k += kRankBlock) {
                const uint64_t v = s_sum[k];
                P.score[d + k] = v;
                top = std::max(top, v);
            }
            d += nd;
        } else {
            // a large document: every lane sums its entries, the workgroup adds the lanes up
            const uint64_t cnt = P.off[d + 1] - e0;
            uint64_t acc = 0;
            for (uint64_t i = tid; i < cnt; i += kRankBlock) {
                const uint32_t t = P.term[e0 + i];
                if (P.distinct && !stats_bitset_first(bits, t)) continue;
                acc += !P.weights ? 1u : w_lds ? s_w[t] : P.weights[t];
            }
            acc = wave_sum64(acc);
            if ((tid & 63u) == 0) s_red[tid >> 6] = acc;
            __syncthreads();                                        // (and: every bit is set before the first is cleared)
            if (P.distinct)
                for (uint64_t i = tid; i < cnt; i += kRankBlock) bits[P.term[e0 + i] >> 5] = 0;   // the words it set, and only those
            if (tid == 0) {
                uint64_t v = 0;
                for (uint32_t w = 0; w < kRankBlock / 64; w++) v += s_red[w];
                P.score[d] = v;
                top = std::max(top, v);
            }
            d += 1;
        }
        __syncthreads();
    }
    top = wave_max64(top);
    if ((tid & 63u) == 0 && top) atomicMax(reinterpret_cast<ull*>(P.ctl + kRankCtlMax), (ull)top);
}

__global__ void __launch_bounds__(kRankBlock) k_top_max(const TopParams P) {
    const uint64_t stride = (uint64_t)gridDim.x * kRankBlock;
    uint64_t top = 0;
    for (uint64_t d = (uint64_t)blockIdx.x * kRankBlock + threadIdx.x; d < P.n_docs; d += stride) top = std::max(top, P.score[d]);
    top = wave_max64(top);
    if ((threadIdx.x & 63u) == 0 && top) atomicMax(reinterpret_cast<ull*>(P.ctl + kRankCtlMax), (ull)top);
}

// (a workgroup's share of the array is far below 2^32 documents: the grid has eight workgroups a compute unit and the array lies
// in device memory)
__global__ void __launch_bounds__(kRankBlock) k_top_hist(const TopParams P) {
    __shared__ uint32_t s_bin[kRankBins];
    for (uint32_t b = threadIdx.x; b < kRankBins; b += kRankBlock) s_bin[b] = 0;
    __syncthreads();
    const uint64_t prefix = P.ctl[kRankCtlPrefix], stride = (uint64_t)gridDim.x * kRankBlock;
    for (uint64_t d = (uint64_t)blockIdx.x * kRankBlock + threadIdx.x; d < P.n_docs; d += stride) {
        const uint64_t key = P.score[d];
        if (rank_in_prefix(key, prefix, P.shift)) atomicAdd(&s_bin[rank_digit(key, P.shift)], 1u);
    }
    __syncthreads();
    uint64_t* const row = P.hist + (uint64_t)(P.shift / kRankDigitBits) * kRankBins;
    for (uint32_t b = threadIdx.x; b < kRankBins; b += kRankBlock)
        if (s_bin[b]) atomicAdd(reinterpret_cast<ull*>(row + b), (ull)s_bin[b]);
}

__global__ void __launch_bounds__(64) k_top_pick(const TopParams P) {
    const uint32_t lane = threadIdx.x;
    const uint64_t* const row = P.hist + (uint64_t)(P.shift / kRankDigitBits) * kRankBins;
    uint64_t cnt[kRankPickBins], mine = 0;
#pragma unroll
    for (uint32_t j = 0; j < kRankPickBins; j++) { cnt[j] = row[rank_pick_bin(lane, j)]; mine += cnt[j]; }
    uint64_t incl = mine;
#pragma unroll
    for (uint32_t s = 1; s < 64; s <<= 1) {
        const uint64_t v = up64(incl, s);
        if (lane >= s) incl += v;
    }
    uint64_t krem = P.ctl[kRankCtlKrem];
    const uint64_t prefix = P.ctl[kRankCtlPrefix], above = incl - mine;
    if (above < krem && krem <= incl) {                             // (one lane)
        const uint32_t digit = rank_pick_in_lane(cnt, lane, above, krem);
        P.ctl[kRankCtlPrefix] = prefix | (uint64_t)digit << P.shift;
        P.ctl[kRankCtlKrem] = krem;
    }
}

// a tile's ballots: cls[j] of the lane's document of trip j, the wave's two masks per trip
struct TileMasks {
    uint64_t gt[kRankPlaceTrips], eq[kRankPlaceTrips], score[kRankPlaceTrips];
};
__device__ __forceinline__ void tile_masks(const TopParams& P, uint64_t tile, uint64_t T, TileMasks& M) {
#pragma unroll
    for (uint32_t j = 0; j < kRankPlaceTrips; j++) {
        const uint64_t d = rank_place_doc(tile, j, threadIdx.x);
        M.score[j] = d < P.n_docs ? P.score[d] : 0;
        const uint32_t cls = d < P.n_docs ? rank_class(M.score[j], T) : 0u;
        M.gt[j] = __ballot(cls == 2u);
        M.eq[j] = __ballot(cls == 1u);
    }
}

__global__ void __launch_bounds__(kRankBlock) k_top_count(const TopParams P) {
    __shared__ uint32_t s_cnt[2];
    const uint64_t T = P.ctl[kRankCtlPrefix];
    for (uint64_t tile = blockIdx.x; tile < P.n_tiles; tile += gridDim.x) {
        if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
        __syncthreads();
        TileMasks M;
        tile_masks(P, tile, T, M);
        uint32_t gt = 0, eq = 0;
#pragma unroll
        for (uint32_t j = 0; j < kRankPlaceTrips; j++) { gt += (uint32_t)__popcll(M.gt[j]); eq += (uint32_t)__popcll(M.eq[j]); }
        if ((threadIdx.x & 63u) == 0) {
            if (gt) atomicAdd(&s_cnt[0], gt);
            if (eq) atomicAdd(&s_cnt[1], eq);
        }
        __syncthreads();
        if (threadIdx.x == 0) { P.tile_gt[tile] = s_cnt[0]; P.tile_eq[tile] = s_cnt[1]; }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kRankBlock) k_top_place(const TopParams P) {
    __shared__ uint32_t s_gt[kRankPlaceRows], s_eq[kRankPlaceRows];
    const uint64_t T = P.ctl[kRankCtlPrefix], c = P.gt_pos[P.n_tiles], keep = rank_equals_kept(P.k, c, P.eq_pos[P.n_tiles]);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t below = lane ? ~0ull >> (64 - lane) : 0;         // the lanes in front of this one
    for (uint64_t tile = blockIdx.x; tile < P.n_tiles; tile += gridDim.x) {
        const uint64_t g0 = P.gt_pos[tile], q0 = P.eq_pos[tile];
        if (P.gt_pos[tile + 1] == g0 && (P.eq_pos[tile + 1] == q0 || q0 >= keep)) continue;   // (the same in every lane)
        TileMasks M;
        tile_masks(P, tile, T, M);
        if (lane == 0) {
#pragma unroll
            for (uint32_t j = 0; j < kRankPlaceTrips; j++) {
                s_gt[rank_place_row(j, wave)] = (uint32_t)__popcll(M.gt[j]);
                s_eq[rank_place_row(j, wave)] = (uint32_t)__popcll(M.eq[j]);
            }
        }
        __syncthreads();
#pragma unroll
        for (uint32_t j = 0; j < kRankPlaceTrips; j++) {
            const bool is_gt = M.gt[j] >> lane & 1, is_eq = M.eq[j] >> lane & 1;
            if (!is_gt && !is_eq) continue;
            const uint32_t row = rank_place_row(j, wave);
            uint64_t r = is_gt ? g0 : q0;
            for (uint32_t k = 0; k < row; k++) r += is_gt ? s_gt[k] : s_eq[k];
            r += (uint32_t)__popcll((is_gt ? M.gt[j] : M.eq[j]) & below);
            if (!is_gt && r >= keep) continue;
            const uint64_t slot = is_gt ? r : c + r;
            if (slot >= P.k) continue;                              // (never: at most k - 1 scores lie above the k-th largest)
            P.cand_score[slot] = M.score[j];
            P.cand_idx[slot] = rank_place_doc(tile, j, threadIdx.x);
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kRankSortBlock) k_top_sort(const TopParams P) {
    __shared__ uint64_t s_score[kRankMaxK], s_idx[kRankMaxK];
    const uint64_t c = P.gt_pos[P.n_tiles], listed = c + rank_equals_kept(P.k, c, P.eq_pos[P.n_tiles]);
    const uint32_t n = listed < P.k ? (uint32_t)listed : P.k, N = rank_sort_size(n);   // (n <= k <= kRankMaxK)
    for (uint32_t i = threadIdx.x; i < N; i += kRankSortBlock) {
        s_score[i] = i < n ? P.cand_score[i] : 0;
        s_idx[i] = i < n ? P.cand_idx[i] : ~0ull;
    }
    __syncthreads();
    for (uint32_t kk = 2; kk <= N; kk <<= 1)
        for (uint32_t j = kk >> 1; j; j >>= 1) {
            for (uint32_t i = threadIdx.x; i < N; i += kRankSortBlock) {
                uint32_t o;
                bool up;
                if (!rank_sort_pair(i, j, kk, o, up)) continue;
                const uint64_t sa = s_score[i], ia = s_idx[i], sb = s_score[o], ib = s_idx[o];
                if (up ? rank_before(sb, ib, sa, ia) : rank_before(sa, ia, sb, ib)) {
                    s_score[i] = sb; s_idx[i] = ib; s_score[o] = sa; s_idx[o] = ia;
                }
            }
            __syncthreads();
        }
    for (uint32_t i = threadIdx.x; i < n; i += kRankSortBlock) {
        P.top_idx[i] = P.doc_base + s_idx[i];
        P.top_score[i] = s_score[i];
    }
    if (threadIdx.x == 0) P.ctl[kRankCtlNTop] = n;
}

__global__ void __launch_bounds__(kRankGatherBlock) k_gather_place(const GatherParams P) {
    const uint64_t stride = (uint64_t)gridDim.x * kRankGatherBlock, t0 = (uint64_t)blockIdx.x * kRankGatherBlock + threadIdx.x;
    if (t0 == 0) { P.ctl[kRankCtlLo] = P.doc_off[0]; P.ctl[kRankCtlHi] = P.doc_off[P.n_docs]; }
    bool bad = false;
    for (uint64_t j = t0; j < P.m; j += stride) {
        uint64_t d, a = 0, b = 0;
        bool ok = rank_gather_doc(P.idx[j], P.idx_base, P.n_docs, d);
        if (ok) { a = P.doc_off[d]; b = P.doc_off[d + 1]; ok = sel_doc_ok(a, b); }
        P.len[j] = ok ? (uint32_t)(b - a) : 0u;
        P.c_src[j] = ok ? a : 0;
        bad |= !ok;
    }
    if (bad) P.ctl[kRankCtlBadIdx] = 1;
}

// workgroups of a grid-stride pass over n items, per_group of them a workgroup at least: eight a compute unit at most, one at least
unsigned stride_grid(uint64_t n, uint64_t per_group, unsigned n_cus) {
    const uint64_t g = (n + per_group - 1) / per_group;
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(g, (uint64_t)std::max(n_cus, 1u) * 8));
}

}  // namespace

hipError_t launch_score_docs(const ScoreParams& P, hipStream_t st) {
    if (!P.n_docs) return hipSuccess;
    k_score_docs<<<dim3(P.grid), dim3(kRankBlock), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_top_max(const TopParams& P, unsigned n_cus, hipStream_t st) {
    if (!P.n_docs) return hipSuccess;
    k_top_max<<<dim3(stride_grid(P.n_docs, kRankHistDocs, n_cus)), dim3(kRankBlock), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_top_hist(const TopParams& P, unsigned n_cus, hipStream_t st) {
    k_top_hist<<<dim3(stride_grid(P.n_docs, kRankHistDocs, n_cus)), dim3(kRankBlock), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_top_pick(const TopParams& P, hipStream_t st) {
    k_top_pick<<<dim3(1), dim3(64), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_top_count(const TopParams& P, hipStream_t st) {
    if (!P.n_tiles) return hipSuccess;
    k_top_count<<<dim3((unsigned)std::min<uint64_t>(P.n_tiles, 1u << 20)), dim3(kRankBlock), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_top_place(const TopParams& P, hipStream_t st) {
    if (!P.n_tiles) return hipSuccess;
    k_top_place<<<dim3((unsigned)std::min<uint64_t>(P.n_tiles, 1u << 20)), dim3(kRankBlock), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_top_sort(const TopParams& P, hipStream_t st) {
    k_top_sort<<<dim3(1), dim3(kRankSortBlock), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_gather_place(const GatherParams& P, unsigned n_cus, hipStream_t st) {
    k_gather_place<<<dim3(stride_grid(P.m, kRankGatherBlock, n_cus)), dim3(kRankGatherBlock), 0, st>>>(P);
    return hipGetLastError();
}

}  // namespace gft
