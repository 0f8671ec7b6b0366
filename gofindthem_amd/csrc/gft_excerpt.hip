// gft_excerpt.hip -- excerpts: the text around the hit spans, cut and gathered (gft_excerpt_spans_device), gfx950 / wave64.
//
//   (text, doc_off; span_off, span_start, span_len; before, after, flags)  ->  out: the excerpts back to back, exc_off, exc_doc,
//                                                                              exc_start, exc_span_off, span_rel, doc_exc_off
//
//   k_excerpt_ends    one lane: span_off[0], span_off[n_docs], doc_off[0], doc_off[n_docs] -> ctl[kExcCtlEnds ..], which the host reads
//                     back in one copy into its pinned words: how many lanes the passes below get
//   k_excerpt_docs    a lane a document: raises ctl[kExcCtlDocs] for offsets that descend, a document of 4 GiB or more, span offsets
//                     that descend (these ctl[kExcCtlOffs] too: a word a condition, every lane stores the same 1)
//   k_excerpt_window  returns at once when ctl[kExcCtlDocs] is raised.  A workgroup a tile of kExcTile spans, a lane a span: its document by a
//                     binary search over span_off (span_doc_of), the window, the rune snap (at most six byte loads inside the
//                     document), with a snap bit the walk of the two edges to a word or line border (the <true> instantiation,
//                     which only gft_excerpt_spans_snap_device launches), the two checks (ctl[kExcCtlSpans]) -> ws, we, sdoc;
//                     the tile's minimum of ws -> tmin
//   k_excerpt_carry   ONE workgroup of kExcCarryTiles lanes, a lane a tile, the trips from the last to the first: a suffix-minimum
//                     scan of tmin (shuffles inside the waves, LDS between them), exclusive -> carry; the minimum of the trip is
//                     the carry of the trip in front of it
//   k_excerpt_mark    returns at once when ctl[kExcCtlDocs] is raised.  A workgroup a tile: the same scan over ws from carry[tile] -> smin;
//                     head and share from smin, we and the neighbour's we
//   (k_scan_* of gft_kernels.hip: head -> rank, share -> pos; k_excerpt_pack gathers what the host reads back into ctl)
//   k_excerpt_place   a lane a span: the heads store the compact arrays c_off / c_src (complete) and the caller's capped arrays
//   k_excerpt_finish  a lane a span: span_rel from c_src of its excerpt; a lane a document: doc_exc_off from rank
//   (k_select_copy of gft_select.hip over (c_off, c_src, n_exc, min(total, cap_bytes)): a lane a 16-byte chunk of the OUTPUT)
//
// Every launch reads only what an earlier launch stored; no atomics.  What a window, a cut, a tile, a trip and a lane decide is in
// gft_excerpt_piece.hpp, which the host compiles too.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gft_excerpt.hpp"

namespace gft {

namespace {

__device__ __forceinline__ uint64_t shfl_down64(uint64_t v, uint32_t step) {
    return (uint64_t)(uint32_t)__shfl_down((int)(v >> 32), step, 64) << 32 | (uint32_t)__shfl_down((int)(uint32_t)v, step, 64);
}

// a wave's inclusive suffix-minimum scan: lane l ends with the minimum of the lanes l .. 63
__device__ __forceinline__ uint64_t wave_suffix_min(uint64_t v, uint32_t lane) {
#pragma unroll
    for (uint32_t step = 1; step < 64; step <<= 1) v = exc_scan_step(v, shfl_down64(v, step), lane, step);
    return v;
}

// the scan of a workgroup of W waves from `carry`: incl = the minimum of this lane's value, every lane's behind it and the carry;
// excl = the same without this lane's own.  tot: W words of LDS.  Every lane of the workgroup calls this.
template <uint32_t W>
__device__ __forceinline__ void block_suffix_min(uint64_t v, uint64_t carry, uint64_t* tot, uint64_t& incl, uint64_t& excl) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint64_t sc = wave_suffix_min(v, lane);
    const uint64_t next = shfl_down64(sc, 1);
    if (lane == 0) tot[w] = sc;
    __syncthreads();
    const uint64_t later = exc_later(tot, W, (int)w, carry);
    incl = exc_min(sc, later);
    excl = exc_exclusive(next, later, lane);
}

__global__ void k_excerpt_ends(const ExcerptParams P) {
    P.ctl[kExcCtlEnds + 0] = P.V.span_off[0];
    P.ctl[kExcCtlEnds + 1] = P.V.span_off[P.V.n_docs];
    P.ctl[kExcCtlEnds + 2] = P.V.doc_off[0];
    P.ctl[kExcCtlEnds + 3] = P.V.doc_off[P.V.n_docs];
}

__global__ void __launch_bounds__(kExcTile) k_excerpt_docs(const ExcerptParams P) {
    const uint64_t d = (uint64_t)blockIdx.x * kExcTile + threadIdx.x;
    if (d >= P.V.n_docs) return;
    const bool bad_doc = !sel_doc_ok(P.V.doc_off[d], P.V.doc_off[d + 1]), bad_off = P.V.span_off[d + 1] < P.V.span_off[d];
    if (bad_doc || bad_off) P.ctl[kExcCtlDocs] = 1;                 // (refuses the call; the same value from every lane)
    if (bad_off) P.ctl[kExcCtlOffs] = 1;                            // (names the message)
}

// kSnap: the lane walks its two edges to a word or line border behind the rune snap (exc_snap_window), every step a single-byte
// load inside the document, a rune decoded once; the class table stays in global memory.  false: the plain call's pass, and the
// run pass of the mark and replace calls.
template <bool kSnap>
__global__ void __launch_bounds__(kExcTile) k_excerpt_window(const ExcerptParams P) {
    __shared__ uint64_t tot[kExcTile / 64];
    if (P.ctl[kExcCtlDocs]) return;                                 // (the same in every lane of the grid)
    const uint64_t k = (uint64_t)blockIdx.x * kExcTile + threadIdx.x;
    uint64_t ws = kExcNone;
    if (k < P.n_spans) {
        uint64_t d, we;
        if (exc_lane_window_t<kSnap>(P.V, P.s0 + k, d, ws, we)) P.ctl[kExcCtlSpans] = 1;
        P.ws[k] = ws;
        P.we[k] = we;
        P.sdoc[k] = d;
    }
    uint64_t incl, excl;
    block_suffix_min<kExcTile / 64>(ws, kExcNone, tot, incl, excl);
    if (threadIdx.x == 0) P.tmin[blockIdx.x] = incl;
}

__global__ void __launch_bounds__(kExcCarryTiles) k_excerpt_carry(const ExcerptParams P) {
    __shared__ uint64_t tot[kExcCarryTiles / 64];
    const uint64_t n_tiles = exc_tiles(P.n_spans);
    uint64_t carry = kExcNone;
    for (uint64_t trip = exc_trips(n_tiles); trip-- > 0;) {
        const uint64_t t = trip * kExcCarryTiles + threadIdx.x;
        const uint64_t v = t < n_tiles ? P.tmin[t] : kExcNone;
        uint64_t incl, excl;
        block_suffix_min<kExcCarryTiles / 64>(v, carry, tot, incl, excl);
        if (t < n_tiles) P.carry[t] = excl;
        carry = exc_later(tot, kExcCarryTiles / 64, -1, carry);     // (the same in every lane)
        __syncthreads();                                            // (tot is written again by the trip in front)
    }
}

__global__ void __launch_bounds__(kExcTile) k_excerpt_mark(const ExcerptParams P) {
    __shared__ uint64_t tot[kExcTile / 64];
    if (P.ctl[kExcCtlDocs]) return;                                 // (the window pass stored nothing: the same in every lane)
    const uint64_t k = (uint64_t)blockIdx.x * kExcTile + threadIdx.x;
    const bool live = k < P.n_spans;
    uint64_t incl, excl;
    block_suffix_min<kExcTile / 64>(live ? P.ws[k] : kExcNone, P.carry[blockIdx.x], tot, incl, excl);
    if (!live) return;
    const bool first = k == 0 || P.s0 + k == P.V.span_off[P.sdoc[k]];
    const uint64_t we = P.we[k], prev_we = k ? P.we[k - 1] : 0;
    const uint32_t head = exc_is_head(first, prev_we, incl);
    P.smin[k] = incl;
    P.head[k] = head;
    P.share[k] = exc_share(head, we, prev_we, incl);
}

__global__ void k_excerpt_pack(const ExcerptParams P) {
    P.ctl[kExcCtlExc] = P.rank[P.n_spans];
    P.ctl[kExcCtlTotal] = P.pos[P.n_spans];
}

__global__ void __launch_bounds__(kExcTile) k_excerpt_place(const ExcerptParams P) {
    const uint64_t k = (uint64_t)blockIdx.x * kExcTile + threadIdx.x;
    if (k == 0) {
        P.c_off[P.m] = P.total;
        if (P.exc_off && P.m <= P.cap_exc) P.exc_off[P.m] = P.total;
        if (P.exc_span_off && P.m <= P.cap_exc) P.exc_span_off[P.m] = P.s0 + P.n_spans;
    }
    if (k >= P.n_spans || !P.head[k]) return;
    const uint64_t r = P.rank[k], at = P.pos[k], src = P.smin[k], d = P.sdoc[k];
    P.c_off[r] = at;
    P.c_src[r] = src;
    if (r <= P.cap_exc) {
        if (P.exc_off) P.exc_off[r] = at;
        if (P.exc_span_off) P.exc_span_off[r] = P.s0 + k;
    }
    if (r < P.cap_exc) {
        if (P.exc_doc) P.exc_doc[r] = d;
        if (P.exc_start) P.exc_start[r] = (uint32_t)(src - P.V.doc_off[d]);
    }
}

__global__ void __launch_bounds__(kExcTile) k_excerpt_finish(const ExcerptParams P) {
    const uint64_t k = (uint64_t)blockIdx.x * kExcTile + threadIdx.x;
    if (P.span_rel && k < P.n_spans) {
        const uint64_t r = P.rank[k] + P.head[k] - 1;               // the excerpt of span k: the heads up to and with it, less one
        P.span_rel[P.s0 + k] = (uint32_t)(P.V.doc_off[P.sdoc[k]] + P.V.span_start[P.s0 + k] - P.c_src[r]);
    }
    if (P.doc_exc_off && k <= P.V.n_docs) P.doc_exc_off[k] = P.rank[P.V.span_off[k] - P.s0];
}

unsigned blocks_for(uint64_t n) { return (unsigned)std::max<uint64_t>((n + kExcTile - 1) / kExcTile, 1); }

}  // namespace

hipError_t launch_excerpt_ends(const ExcerptParams& P, hipStream_t st) {
    if (!P.V.n_docs) return hipSuccess;
    k_excerpt_ends<<<dim3(1), dim3(1), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_excerpt_docs(const ExcerptParams& P, hipStream_t st) {
    if (!P.V.n_docs) return hipSuccess;
    k_excerpt_docs<<<dim3(blocks_for(P.V.n_docs)), dim3(kExcTile), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_excerpt_window(const ExcerptParams& P, hipStream_t st) {
    if (!P.n_spans) return hipSuccess;
    const dim3 grid((unsigned)exc_tiles(P.n_spans));
    if (P.V.flags & (GFT_EXCERPT_WORDS | GFT_EXCERPT_LINES)) k_excerpt_window<true><<<grid, dim3(kExcTile), 0, st>>>(P);
    else k_excerpt_window<false><<<grid, dim3(kExcTile), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_excerpt_carry(const ExcerptParams& P, hipStream_t st) {
    if (!P.n_spans) return hipSuccess;
    k_excerpt_carry<<<dim3(1), dim3(kExcCarryTiles), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_excerpt_mark(const ExcerptParams& P, hipStream_t st) {
    if (!P.n_spans) return hipSuccess;
    k_excerpt_mark<<<dim3((unsigned)exc_tiles(P.n_spans)), dim3(kExcTile), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_excerpt_pack(const ExcerptParams& P, hipStream_t st) {
    k_excerpt_pack<<<dim3(1), dim3(1), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_excerpt_place(const ExcerptParams& P, hipStream_t st) {
    // (one block at least: thread 0 closes c_off, exc_off and exc_span_off)
    k_excerpt_place<<<dim3(blocks_for(P.n_spans)), dim3(kExcTile), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_excerpt_finish(const ExcerptParams& P, hipStream_t st) {
    if (!P.span_rel && !P.doc_exc_off) return hipSuccess;
    k_excerpt_finish<<<dim3(blocks_for(std::max(P.n_spans, P.V.n_docs + 1))), dim3(kExcTile), 0, st>>>(P);
    return hipGetLastError();
}

}  // namespace gft
