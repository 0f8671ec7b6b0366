// gft_mark.hip -- highlight: markers written round the hit spans (gft_mark_spans_device), gfx950 / wave64.
//
//   (text, doc_off; span_off, span_start, span_len; open, close)  ->  out: the marked documents back to back, out_off, span_new,
//                                                                     doc_run_off
//
//   (k_excerpt_docs, k_excerpt_window, k_excerpt_carry, k_excerpt_mark of gft_excerpt.hip with before = after = 0 and no snap:
//    the checks, every span's interval, the suffix minimum, the heads; k_scan_* of gft_kernels.hip: head -> rank)
//   k_mark_check    a lane a document: raises ctl[kMarkCtlGrow] for a document that reaches 4 GiB once marked; lane 0 leaves the
//                   number of runs in ctl[kExcCtlExc].  The host reads the control block and refuses before anything is written
//   k_mark_place    a lane a span: the heads store q[2r], the last span of a run q[2r + 1]; every span its span_new; a lane a
//                   document: out_off and doc_run_off from rank
//   k_mark_copy     from the OUTPUT side: a wave owns a tile of 4 KiB of the output, a lane a 16-byte chunk aligned to the output
//                   address.  The markers go into LDS once per workgroup.  One uniform binary search per tile over the insertion
//                   positions, then a window of kMarkWindow insertions across the lanes.  EVERY chunk loads its text once --
//                   its text bytes are consecutive in the blob whatever markers lie between them: aligned 16-byte loads and the
//                   byte-align funnel --, the loads of a tile's four trips issued before the first store; a chunk that holds no
//                   insertion -- the common case -- stores them as they are, a chunk that meets insertions spreads them round the
//                   marker bytes segment by segment in registers: the positions from the window's copy in LDS, the marker bytes
//                   as words of the block through the same funnel.  Bytes are stored singly only in the first and the last chunk
//                   of the range.
//
// Every launch reads only what an earlier launch stored; no atomics.  What the insertion list, a window and a chunk decide is in
// gft_mark_piece.hpp, which the host compiles too.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gft_mark.hpp"
#include "gft_wave_dev.hpp"

namespace gft {

namespace {

constexpr uint32_t kMarkBlock = 256;        // 4 waves; the copy pass: a tile each

__global__ void __launch_bounds__(kExcTile) k_mark_check(const MarkParams P) {
    const ExcerptParams& X = P.X;
    const uint64_t d = (uint64_t)blockIdx.x * kExcTile + threadIdx.x;
    if (X.ctl[kExcCtlDocs]) return;                                 // (offsets that descend: nothing behind them is read)
    if (d == 0) X.ctl[kExcCtlExc] = X.rank[X.n_spans];
    if (d >= X.V.n_docs) return;
    const uint64_t r = X.rank[X.V.span_off[d + 1] - X.s0] - X.rank[X.V.span_off[d] - X.s0];
    if (!mark_grow_ok(X.V.doc_off[d + 1] - X.V.doc_off[d], r, P.M.ol, P.M.cl)) X.ctl[kMarkCtlGrow] = 1;
}

__global__ void __launch_bounds__(kExcTile) k_mark_place(const MarkParams P) {
    const ExcerptParams& X = P.X;
    const uint64_t k = (uint64_t)blockIdx.x * kExcTile + threadIdx.x;
    if (k < X.n_spans) {
        const uint32_t head = X.head[k];
        const uint64_t r = X.rank[k] + head - 1, d = X.sdoc[k];     // the run of span k: the heads up to and with it, less one
        if (head) P.q[2 * r] = X.smin[k];
        if (k + 1 == X.n_spans || X.head[k + 1]) P.q[2 * r + 1] = X.we[k];
        if (P.span_new)
            P.span_new[X.s0 + k] = mark_span_new(X.V.span_start[X.s0 + k], r - X.rank[X.V.span_off[d] - X.s0], P.M.ol, P.M.cl);
    }
    if (k <= X.V.n_docs && (P.out_off || P.doc_run_off)) {
        const uint64_t r = X.rank[X.V.span_off[k] - X.s0];
        if (P.doc_run_off) P.doc_run_off[k] = r;
        if (P.out_off) P.out_off[k] = X.V.doc_off[k] - P.M.base + r * ((uint64_t)P.M.ol + P.M.cl);
    }
}

// the window across the lanes as mark_lift reads it
struct WindowRel {
    uint32_t mine;
    __device__ __forceinline__ uint32_t operator()(uint32_t w) const { return (uint32_t)__shfl((int)mine, (int)w, 64); }
};

__global__ void __launch_bounds__(kMarkBlock) k_mark_copy(const MarkParams P) {
    __shared__ uint64_t marks[kMarkWords];
    __shared__ uint32_t wrel[kMarkBlock / 64][kMarkWindow];
    if (threadIdx.x < kMarkWords) marks[threadIdx.x] = P.marks[threadIdx.x];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wv = first_lane32(threadIdx.x >> 6);
    const uint64_t tile = (uint64_t)blockIdx.x * (kMarkBlock / 64) + wv;
    const SelGeom G = P.G;
    const MarkPlan M = P.M;
    const bool live = tile < sel_tiles(G);                          // (the same in every lane of the wave)
    const uint64_t c0 = tile * (kSelTile / kSelChunk);
    uint64_t lo[kSelTrips], hi[kSelTrips];
    MarkCursor cur[kSelTrips];
    SelV acc[kSelTrips];
    uint64_t tile_lo = 0, tile_hi = 0, nb = 0;
    uint64_t front = 0;
    WindowRel win{0xFFFFFFFFu};
    if (live) {
        sel_chunk_range(G, c0, tile_lo, tile_hi);
        // the insertions at or in front of the tile's first byte: uniform, searched on scalar values
        nb = first_lane64(mark_count(M, tile_lo));
        win.mine = mark_window_rel(M, nb, lane, tile_lo);
        front = first_lane64(mark_window_front(M, nb));
    }
    wrel[wv][lane] = win.mine;                                      // (the window once more in LDS: what a chunk that meets insertions reads)
    __syncthreads();                                                // (every wave of the workgroup, the ones past the range too)
    if (!live) return;
    const MarkWin W{wrel[wv], nb, tile_lo};
    SelV T[kSelTrips];
    bool rest[kSelTrips];
#pragma unroll
    for (uint32_t t = 0; t < kSelTrips; t++) {
        const uint64_t c = c0 + t * 64u + lane;
        sel_chunk_range(G, c, lo[t], hi[t]);
        const bool valid = lo[t] < hi[t];
        const uint32_t lo_rel = valid ? (uint32_t)(lo[t] - tile_lo) : 0u, hi_rel = valid ? (uint32_t)(hi[t] - tile_lo) : 0u;
        const uint32_t cnt = mark_lift(win, lo_rel);
        const uint32_t prev_rel = win(cnt ? cnt - 1 : 0), next_rel = win(cnt);  // (every lane makes both calls)
        const bool shown = cnt < kMarkWindow - 1;
        uint64_t n = nb + cnt, prev_at = cnt ? tile_lo + prev_rel : front;
        if (valid && !shown) {                                      // (the window does not say: this lane searches the list)
            n = mark_count(M, lo[t]);
            prev_at = mark_at(M, n - 1);
        }
        const uint32_t j = sel_chunk_byte(G, c, lo[t]);
        acc[t] = T[t] = SelV{0, 0};
        cur[t] = MarkCursor{lo[t], n, j};
        rest[t] = false;
        if (valid) {
            T[t] = mark_chunk_text(M, P.X.V.text, mark_chunk_src(M, n, prev_at, lo[t]), lo[t], hi[t]);
            rest[t] = !(shown && mark_chunk_plain(M, n, prev_at, lo[t], next_rel, hi_rel));
        }
    }
#pragma unroll
    for (uint32_t t = 0; t < kSelTrips; t++) {
        if (rest[t]) mark_chunk_rest(M, W, T[t], marks, hi[t], cur[t], acc[t]);
        else acc[t] = sel_shift(T[t], cur[t].j);
    }
#pragma unroll
    for (uint32_t t = 0; t < kSelTrips; t++) {
        const uint64_t c = c0 + t * 64u + lane;
        if (lo[t] < hi[t]) sel_store(P.out, G, c, lo[t], hi[t], acc[t]);
    }
}

unsigned blocks_for(uint64_t n) { return (unsigned)std::max<uint64_t>((n + kExcTile - 1) / kExcTile, 1); }

}  // namespace

hipError_t launch_mark_check(const MarkParams& P, hipStream_t st) {
    if (!P.X.V.n_docs) return hipSuccess;
    k_mark_check<<<dim3(blocks_for(P.X.V.n_docs)), dim3(kExcTile), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_mark_place(const MarkParams& P, hipStream_t st) {
    if (!P.X.V.n_docs) return hipSuccess;
    k_mark_place<<<dim3(blocks_for(std::max(P.X.n_spans, P.X.V.n_docs + 1))), dim3(kExcTile), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_mark_copy(const MarkParams& P, hipStream_t st) {
    const uint64_t tiles = sel_tiles(P.G);
    if (!tiles) return hipSuccess;
    k_mark_copy<<<dim3((unsigned)((tiles + kMarkBlock / 64 - 1) / (kMarkBlock / 64))), dim3(kMarkBlock), 0, st>>>(P);
    return hipGetLastError();
}

}  // namespace gft
