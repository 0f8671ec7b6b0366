// gft_stats.hip -- term statistics of a match or span list (gft_term_stats_device) and column counts of a hit bitmap
// (gft_count_columns_device), gfx950 / wave64.
//
//   (off, term)  ->  occ[t], docs[t], first[t]          bitmap rows  ->  count[c]
//
//   k_stats_check    grid-stride: raises ctl[kStatsCtlOffs] for an offset that descends, ctl[kStatsCtlTerms] for a term id that is
//                    no index of the counters.  Every later launch returns at once when either is set: a refused call writes nothing
//   k_stats_init     (without GFT_STATS_ACCUMULATE) 0, 0, UINT64_MAX into the counters
//   k_stats_count    a workgroup owns a range of whole documents of near-equal weight (stats_cut) and walks it in steps
//                    (gft_stats_piece.hpp): the step's offsets into LDS, a lane an entry, the entry's document by a search in those
//                    offsets, "first of its term in its document" by compare-and-swap on the step's set in LDS -- for a document of
//                    kStatsLarge entries or more by test-and-set on a bitset, in LDS or in the workgroup's global row --, then the
//                    workgroup's cache in LDS: 32-bit adds and a 64-bit minimum per entry, one global 64-bit atomic per (workgroup,
//                    term, counter) when the slot is evicted or the range ends.  The hot terms never leave LDS in between
//   k_count_columns  a workgroup owns kStatsColRows rows of one word column: a lane a row, a ballot per bit, the four waves' sums
//                    combined in LDS, one global atomic per (workgroup, column)
//
// Counters are written by vector atomics and plain vector stores only.  The check pass is what keeps the atomics inside the
// counters: the count pass never runs on a list that failed it.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gft_stats.hpp"
#include "gft_stats_dev.hpp"

namespace gft {

namespace {

constexpr uint32_t kTrips = kStatsStep / kStatsBlock;
constexpr uint64_t kNoDoc = ~0ull;
typedef unsigned long long ull;

__global__ void __launch_bounds__(kStatsBlock) k_stats_check(const StatsParams P) {
    const uint64_t stride = (uint64_t)gridDim.x * kStatsBlock, t0 = (uint64_t)blockIdx.x * kStatsBlock + threadIdx.x;
    bool bad_off = false, bad_term = false;
    for (uint64_t d = t0; d < P.n_docs; d += stride) bad_off |= P.off[d + 1] < P.off[d];
    for (uint64_t i = t0; i < P.n; i += stride) bad_term |= P.term[P.e0 + i] >= P.n_terms;
    if (bad_off) P.ctl[kStatsCtlOffs] = 1;
    if (bad_term) P.ctl[kStatsCtlTerms] = 1;
}

__global__ void __launch_bounds__(kStatsBlock) k_stats_init(const StatsParams P) {
    if (P.ctl[kStatsCtlOffs] | P.ctl[kStatsCtlTerms]) return;
    const uint64_t t = (uint64_t)blockIdx.x * kStatsBlock + threadIdx.x;
    if (t >= P.n_terms) return;
    if (P.occ) P.occ[t] = 0;
    if (P.docs) P.docs[t] = 0;
    if (P.first) P.first[t] = kNoDoc;
}

struct Cache {
    uint32_t* term;
    uint32_t* occ;
    uint32_t* docs;
    uint32_t* flag;
    uint64_t* first;
};

__device__ __forceinline__ void to_global(const StatsParams& P, uint32_t t, uint32_t o, uint32_t dc, uint64_t f) {
    if (P.occ && o) atomicAdd(reinterpret_cast<ull*>(P.occ + t), (ull)o);
    if (P.docs && dc) atomicAdd(reinterpret_cast<ull*>(P.docs + t), (ull)dc);
    if (P.first && f != kNoDoc) atomicMin(reinterpret_cast<ull*>(P.first + t), (ull)f);
}

__device__ __forceinline__ void cache_add(const Cache& C, uint32_t s, bool fst, uint64_t doc) {
    atomicAdd(&C.occ[s], 1u);
    if (fst) {
        atomicAdd(&C.docs[s], 1u);
        atomicMin(reinterpret_cast<ull*>(&C.first[s]), (ull)doc);
    }
}

__device__ __forceinline__ void cache_reset(const Cache& C, uint32_t s, uint32_t t) {
    C.term[s] = t; C.occ[s] = 0; C.docs[s] = 0; C.first[s] = kNoDoc;
}

// every slot to the global counters; the cache is empty afterwards
__device__ void cache_flush(const StatsParams& P, const Cache& C) {
    for (uint32_t s = threadIdx.x; s < kStatsCacheSlots; s += kStatsBlock) {
        const uint32_t t = C.term[s];
        if (t == kStatsNoTerm) continue;
        to_global(P, t, C.occ[s], C.docs[s], C.first[s]);
        cache_reset(C, s, kStatsNoTerm);
    }
    __syncthreads();
}

// a step's entries, a lane kTrips of them (live: bit j), into the cache; every lane of the workgroup calls it
__device__ __forceinline__ void cache_step(const StatsParams& P, const Cache& C, uint32_t live, const uint32_t (&t)[kTrips], uint32_t fst,
                                           const uint64_t (&doc)[kTrips]) {
#ifdef GFT_STATS_NO_COMBINE
    // the study variant of tools/bench_term_stats.py (never in the library): one global atomic per entry and counter
#pragma unroll
    for (uint32_t j = 0; j < kTrips; j++)
        if (live >> j & 1) to_global(P, t[j], 1, fst >> j & 1, (fst >> j & 1) ? doc[j] : kNoDoc);
    __syncthreads();
    return;
#endif
    uint32_t conf = 0, won = 0;
#pragma unroll
    for (uint32_t j = 0; j < kTrips; j++) {
        if (!(live >> j & 1)) continue;
        const uint32_t s = stats_cache_slot(t[j]);
        const uint32_t old = atomicCAS(&C.term[s], kStatsNoTerm, t[j]);
        if (old == kStatsNoTerm || old == t[j]) cache_add(C, s, fst >> j & 1, doc[j]);
        else conf |= 1u << j;
    }
    __syncthreads();
    // a slot that holds another term: one of the lanes that met it evicts it and installs its own
#pragma unroll
    for (uint32_t j = 0; j < kTrips; j++) {
        if (!(conf >> j & 1)) continue;
        const uint32_t s = stats_cache_slot(t[j]);
        if (atomicExch(&C.flag[s], 1u) != 0) continue;
        won |= 1u << j;
        to_global(P, C.term[s], C.occ[s], C.docs[s], C.first[s]);
        cache_reset(C, s, t[j]);
    }
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < kTrips; j++) {
        if (!(conf >> j & 1)) continue;
        const uint32_t s = stats_cache_slot(t[j]);
        const bool f = fst >> j & 1;
        if (C.term[s] == t[j]) cache_add(C, s, f, doc[j]);
        else to_global(P, t[j], 1, f, f ? doc[j] : kNoDoc);      // (a third term of the slot in one step)
        if (won >> j & 1) C.flag[s] = 0;
    }
    __syncthreads();
}

__global__ void __launch_bounds__(kStatsBlock) k_stats_count(const StatsParams P) {
    __shared__ uint64_t s_set[kStatsSetSlots];                      // the step's set; the large path's bitset
    __shared__ uint64_t c_first[kStatsCacheSlots];
    __shared__ uint32_t c_term[kStatsCacheSlots], c_occ[kStatsCacheSlots], c_docs[kStatsCacheSlots], c_flag[kStatsCacheSlots];
    __shared__ uint32_t s_rel[kStatsStepDocs + 1];
    if (P.ctl[kStatsCtlOffs] | P.ctl[kStatsCtlTerms]) return;       // (the same in every lane)
    const uint32_t tid = threadIdx.x;
    const Cache C{c_term, c_occ, c_docs, c_flag, c_first};
    for (uint32_t s = tid; s < kStatsSetSlots; s += kStatsBlock) s_set[s] = 0;
    for (uint32_t s = tid; s < kStatsCacheSlots; s += kStatsBlock) { cache_reset(C, s, kStatsNoTerm); c_flag[s] = 0; }
    __syncthreads();
    const uint64_t dlo = stats_cut(P.off, P.n_docs, blockIdx.x, P.grid), dhi = stats_cut(P.off, P.n_docs, blockIdx.x + 1u, P.grid);
    uint32_t* const bits = P.rows ? P.rows + (uint64_t)blockIdx.x * stats_bitset_words(P.n_terms) : reinterpret_cast<uint32_t*>(s_set);
    uint64_t since = 0;                                             // entries since the cache was last empty
    uint32_t t[kTrips];
    uint64_t doc[kTrips];
    for (uint64_t d = dlo; d < dhi;) {
        const uint64_t e0 = P.off[d];
        const uint32_t tries = dhi - d < kStatsStepDocs ? (uint32_t)(dhi - d) : kStatsStepDocs;
        for (uint32_t k = tid; k <= tries; k += kStatsBlock) s_rel[k] = stats_rel(P.off[d + k], e0);
        __syncthreads();
        const LdsRel rel{s_rel};
        const uint32_t nd = stats_step_docs(rel, tries);
        if (nd) {
            const uint32_t ne = s_rel[nd];
            if (ne) {
                if (since + ne > kStatsFlushEntries) { cache_flush(P, C); since = 0; }
                since += ne;
                uint32_t live = 0, fst = 0, mine[kTrips];
#pragma unroll
                for (uint32_t j = 0; j < kTrips; j++) {
                    const uint32_t i = j * kStatsBlock + tid;
                    t[j] = 0; doc[j] = 0; mine[j] = 0;
                    if (i >= ne) continue;
                    live |= 1u << j;
                    t[j] = P.term[e0 + i];
                    const uint32_t dl = stats_find_doc(rel, nd, i);
                    doc[j] = P.doc_base + d + dl;
                    if (stats_set_first(s_set, dl, t[j], mine[j])) fst |= 1u << j;
                }
                __syncthreads();                                    // (every key is in the set before the first is taken out)
#pragma unroll
                for (uint32_t j = 0; j < kTrips; j++)
                    if (fst >> j & 1) s_set[mine[j]] = 0;           // the set is empty again for the next step
                cache_step(P, C, live, t, fst, doc);
            }
            d += nd;
        } else {
            // a large document: kStatsStep entries at a time, the bitset says which entry is the first of its term
            const uint64_t cnt = P.off[d + 1] - e0;
            for (uint64_t c0 = 0; c0 < cnt; c0 += kStatsStep) {
                const uint32_t ne = cnt - c0 < kStatsStep ? (uint32_t)(cnt - c0) : kStatsStep;
                if (since + ne > kStatsFlushEntries) { cache_flush(P, C); since = 0; }
                since += ne;
                uint32_t live = 0, fst = 0;
#pragma unroll
                for (uint32_t j = 0; j < kTrips; j++) {
                    const uint32_t i = j * kStatsBlock + tid;
                    t[j] = 0; doc[j] = P.doc_base + d;
                    if (i >= ne) continue;
                    live |= 1u << j;
                    t[j] = P.term[e0 + c0 + i];
                    if (stats_bitset_first(bits, t[j])) fst |= 1u << j;
                }
                cache_step(P, C, live, t, fst, doc);
            }
            for (uint64_t i = tid; i < cnt; i += kStatsBlock) bits[P.term[e0 + i] >> 5] = 0;   // the words it set, and only those
            d += 1;
        }
        __syncthreads();
    }
    cache_flush(P, C);
}

__global__ void __launch_bounds__(kStatsBlock) k_count_columns(const ColumnParams P) {
    __shared__ uint32_t s_cnt[32];
    const uint32_t tid = threadIdx.x, W = stats_col_words(P.n_cols), w = blockIdx.x % W, mask = stats_col_mask(P.n_cols, w);
    if (tid < 32) s_cnt[tid] = 0;
    __syncthreads();
    uint32_t cnt[32];
#pragma unroll
    for (uint32_t b = 0; b < 32; b++) cnt[b] = 0;
    const uint64_t r0 = (uint64_t)(blockIdx.x / W) * kStatsColRows;
    for (uint32_t it = 0; it < kStatsColRows / kStatsBlock; it++) {
        const uint64_t r = r0 + it * kStatsBlock + tid;
        uint32_t word = 0;
        if (r < P.n_rows) word = P.bitmap[(P.row_idx ? P.row_idx[r] : r) * W + w] & mask;
#pragma unroll
        for (uint32_t b = 0; b < 32; b++) cnt[b] += (uint32_t)__popcll(__ballot(word >> b & 1u));   // (wave-uniform sums)
    }
    const uint32_t lane = tid & 63u;
    uint32_t mine = 0;
#pragma unroll
    for (uint32_t b = 0; b < 32; b++) mine = lane == b ? cnt[b] : mine;
    if (lane < 32 && mine) atomicAdd(&s_cnt[lane], mine);
    __syncthreads();
    if (tid < 32 && s_cnt[tid]) atomicAdd(reinterpret_cast<ull*>(P.count + (uint64_t)w * 32 + tid), (ull)s_cnt[tid]);
}

}  // namespace

uint32_t stats_resident(unsigned n_cus) { return std::max(n_cus, 1u) * 3u; }   // (44 KB of LDS a workgroup: three on a compute unit)

hipError_t launch_stats_check(const StatsParams& P, unsigned n_cus, hipStream_t st) {
    const uint64_t m = std::max(P.n, P.n_docs);
    if (!m) return hipSuccess;
    const uint64_t g = std::min<uint64_t>((m + kStatsBlock - 1) / kStatsBlock, (uint64_t)std::max(n_cus, 1u) * 8);
    k_stats_check<<<dim3((unsigned)g), dim3(kStatsBlock), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_stats_init(const StatsParams& P, hipStream_t st) {
    if (!P.n_terms) return hipSuccess;
    k_stats_init<<<dim3((unsigned)(((uint64_t)P.n_terms + kStatsBlock - 1) / kStatsBlock)), dim3(kStatsBlock), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_stats_count(const StatsParams& P, hipStream_t st) {
    if (!P.n) return hipSuccess;
    k_stats_count<<<dim3(P.grid), dim3(kStatsBlock), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_count_columns(const ColumnParams& P, hipStream_t st) {
    if (!P.n_rows || !P.n_cols) return hipSuccess;
    const uint64_t gx = (P.n_rows + kStatsColRows - 1) / kStatsColRows;
    k_count_columns<<<dim3((unsigned)(gx * stats_col_words(P.n_cols))), dim3(kStatsBlock), 0, st>>>(P);   // (the caller keeps this below 2^31)
    return hipGetLastError();
}

}  // namespace gft
