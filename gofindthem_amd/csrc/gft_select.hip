// gft_select.hip -- the documents that matched, gathered into one blob (gft_select_docs_device), gfx950 / wave64.
//
//   (text, doc_off, hit rows, want, mode, also)  ->  out: the selected documents back to back, out_off, doc_idx
//
//   k_select_mark   reads the rows with join_bit_rows of gft_bitrows_dev.hpp (the lanes of a wave on consecutive words: 64 / W'
//                   rows per wave for W <= 64, a row per wave in steps of 64 words above that), joins (any, all) against
//                   `want` over the row, applies the mode and `also`
//                   -> len[d], sel[d]; raises ctl[kSelCtlFlag] for offsets that descend or a document of 4 GiB or more
//   (k_scan_* of gft_kernels.hip: len -> pos, sel -> rank; k_select_pack gathers what the host reads back into ctl)
//   k_select_place  a thread a document: the compact arrays c_off / c_src (complete), the caller's out_off / doc_idx (capped)
//   k_select_copy   from the OUTPUT side: a wave owns a tile of 4 KiB of the output, a lane a 16-byte chunk aligned to the output
//                   address per trip.  Per tile one binary search over c_off for a uniform value (sel_search, on scalar values); a window of 64 compact documents
//                   across the lanes (start relative to the tile in 32 bits, and text-minus-output delta) answers "which document
//                   is my chunk's first byte in, where does it end, where does it come from" with shuffles alone -- no lane loads
//                   an offset of its own -- and slides when the documents are shorter than the chunks.  The first segments of the
//                   four trips are loaded (aligned 16-byte granules, byte-align funnel) before anything is stored; chunks that
//                   meet further documents finish in a loop of their own.
//
// Every launch reads only what an earlier launch stored; no atomics.  What a row, a chunk and a window say is decided by
// gft_select_piece.hpp, which the host compiles too.  Memory bound: one read and one write of the bytes copied.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gft_bitrows_dev.hpp"
#include "gft_kernels.hpp"
#include "gft_select.hpp"

namespace gft {

namespace {

constexpr uint32_t kSelBlock = kBitRowsBlock;   // 4 waves; the copy pass: a tile each

// what join_bit_rows joins over a row: (any, all) of the row's words against the same words of `want`
struct SelectSink {
    using Value = SelRow;
    using Col = uint32_t;
    const SelectParams& P;
    __device__ __forceinline__ SelRow identity() const { return SelRow{0, 1}; }
    __device__ __forceinline__ uint32_t column(uint32_t j) const { return P.want[j]; }
    __device__ __forceinline__ SelRow word(uint32_t w, uint32_t want) const { return sel_row_word(w, want); }
    __device__ __forceinline__ SelRow join(SelRow a, SelRow b) const { return sel_row_join(a, b); }
    __device__ __forceinline__ SelRow exchange(SelRow r, uint32_t s) const {
        return SelRow{(uint32_t)__shfl_xor((int)r.any, (int)s, 64), (uint32_t)__shfl_xor((int)r.all, (int)s, 64)};
    }
    __device__ __forceinline__ void finish(uint64_t row, SelRow r) const {
        uint32_t s = sel_row_decide(r, P.mode);
        if (P.also && P.also[row]) s = 1;
        const uint64_t a = P.doc_off[row], b = P.doc_off[row + 1];
        const uint32_t ok = sel_doc_ok(a, b);
        if (!ok) P.ctl[kSelCtlFlag] = 1;
        P.len[row] = (s && ok) ? (uint32_t)(b - a) : 0u;
        P.sel[row] = s;
    }
};

__global__ void __launch_bounds__(kSelBlock) k_select_mark(const SelectParams P) {
    const SelectSink S{P};
    if (P.W == 0) {
        const uint64_t thread = (uint64_t)blockIdx.x * kSelBlock + threadIdx.x, n_threads = (uint64_t)gridDim.x * kSelBlock;
        for (uint64_t row = thread; row < P.n_docs; row += n_threads) S.finish(row, S.identity());
    } else {
        join_bit_rows(BitRows{P.bitmap, P.n_docs, P.W, P.lg, 0}, S);
    }
}

__global__ void k_select_pack(const SelectParams P) {
    P.ctl[kSelCtlTotal] = P.pos[P.n_docs];
    P.ctl[kSelCtlM] = P.rank[P.n_docs];
    P.ctl[kSelCtlLo] = P.doc_off[0];
    P.ctl[kSelCtlHi] = P.doc_off[P.n_docs];
}

__global__ void __launch_bounds__(kSelBlock) k_select_place(const SelectParams P) {
    const uint64_t d = (uint64_t)blockIdx.x * kSelBlock + threadIdx.x;
    uint64_t r;
    if (d == 0) sel_place_close(P, P.m, P.total);
    if (d < P.n_docs) sel_place_doc(P, d, r);
}

// the window across the lanes as sel_lift reads it
struct WindowRel {
    uint32_t mine;
    __device__ __forceinline__ uint32_t operator()(uint32_t j) const { return (uint32_t)__shfl((int)mine, (int)j, 64); }
};

__global__ void __launch_bounds__(kSelBlock) k_select_copy(const SelectParams P) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wv = first_lane32(threadIdx.x >> 6);
    const uint64_t tile = (uint64_t)blockIdx.x * (kSelBlock / 64) + wv;
    const SelGeom G = P.G;
    if (tile >= sel_tiles(G)) return;                               // (the same in every lane)
    const uint64_t c0 = tile * (kSelTile / kSelChunk);
    uint64_t lo[kSelTrips], hi[kSelTrips], p[kSelTrips], k[kSelTrips];
    SelV acc[kSelTrips];
    uint64_t tile_lo, tile_hi;
    sel_chunk_range(G, c0, tile_lo, tile_hi);
    // the compact document of the tile's first byte: uniform, searched on scalar values
    uint64_t kbase = first_lane64(sel_search(P.c_off, P.m, tile_lo));
    WindowRel win{sel_window_rel(P.c_off, P.m, kbase, lane, tile_lo)};
    uint64_t delta = sel_window_delta(P.c_off, P.c_src, P.m, kbase, lane);
#pragma unroll
    for (uint32_t t = 0; t < kSelTrips; t++) {
        const uint64_t c = c0 + t * 64u + lane;
        sel_chunk_range(G, c, lo[t], hi[t]);
        const bool valid = lo[t] < hi[t];
        const uint32_t p_rel = valid ? (uint32_t)(lo[t] - tile_lo) : 0u;
        bool need = valid;
        uint64_t doc_delta = 0;
        uint32_t doc_end = 0;
        k[t] = 0;
        for (;;) {
            const uint32_t idx = sel_lift(win, p_rel);
            const bool ok = idx < kSelWindow - 1;
            const uint32_t next = win(ok ? idx + 1 : idx);
            const uint64_t d = shuffle64(delta, (int)idx);
            if (need && ok) { k[t] = kbase + idx; doc_end = next; doc_delta = d; }
            const uint64_t newly = __ballot(need && ok);
            need = need && !ok;
            const uint64_t left = __ballot(need);
            if (!left) break;                                       // (the same in every lane)
            // the documents are shorter than the chunks: slide; where a whole window resolved nobody, search again
            if (newly) kbase += kSelWindow - 1;
            else kbase = first_lane64(sel_search(P.c_off, P.m, lane_value64(lo[t], __builtin_ctzll(left))));
            win.mine = sel_window_rel(P.c_off, P.m, kbase, lane, tile_lo);
            delta = sel_window_delta(P.c_off, P.c_src, P.m, kbase, lane);
        }
        acc[t] = SelV{0, 0};
        p[t] = lo[t];
        if (valid) p[t] = sel_segment_at(P.text, doc_delta, tile_lo + doc_end, lo[t], hi[t], sel_chunk_byte(G, c, lo[t]), acc[t]);
    }
#pragma unroll
    for (uint32_t t = 0; t < kSelTrips; t++) {
        const uint64_t c = c0 + t * 64u + lane;
        if (p[t] < hi[t]) sel_more_segments(P.text, P.c_off, P.c_src, k[t], p[t], hi[t], sel_chunk_byte(G, c, p[t]), acc[t]);
    }
#pragma unroll
    for (uint32_t t = 0; t < kSelTrips; t++) {
        const uint64_t c = c0 + t * 64u + lane;
        if (lo[t] < hi[t]) sel_store(P.out, G, c, lo[t], hi[t], acc[t]);
    }
}

}  // namespace

hipError_t launch_select_mark(const SelectParams& P, unsigned n_cus, hipStream_t st) {
    if (!P.n_docs) return hipSuccess;
    k_select_mark<<<dim3(join_rows_grid(BitRows{P.bitmap, P.n_docs, P.W, P.lg, 0}, P.W == 0, n_cus)), dim3(kSelBlock), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_select_pack(const SelectParams& P, hipStream_t st) {
    k_select_pack<<<dim3(1), dim3(1), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_select_place(const SelectParams& P, hipStream_t st) {
    // (one block at least: thread 0 closes c_off and out_off)
    k_select_place<<<dim3((unsigned)std::max<uint64_t>((P.n_docs + kSelBlock - 1) / kSelBlock, 1)), dim3(kSelBlock), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_select_copy(const SelectParams& P, hipStream_t st) {
    const uint64_t tiles = sel_tiles(P.G);
    if (!tiles) return hipSuccess;
    k_select_copy<<<dim3((unsigned)((tiles + kSelBlock / 64 - 1) / (kSelBlock / 64))), dim3(kSelBlock), 0, st>>>(P);
    return hipGetLastError();
}

}  // namespace gft
