// gft_replace.hip -- replace: every hit run rewritten by its replacement (gft_replace_spans_device), gfx950 / wave64.
//
//   (text, doc_off; span_off, span_start, span_len, span_key; key_rep, the table)  ->  out: the replaced documents back to back,
//                                                                                      out_off, doc_run_off, run_new, run_len, run_rep
//
//   (k_excerpt_docs, k_excerpt_window, k_excerpt_carry, k_excerpt_mark of gft_excerpt.hip with before = after = 0 and no snap:
//    the checks, every span's interval, the suffix minimum, the heads, every span's share of its run's bytes; k_scan_* of
//    gft_kernels.hip: head -> rank, share -> pos, len -> ppos)
//   k_replace_ids     a lane a span: the id it asks for (ctl[kRepCtlKey] for a key or an id out of range), atomicMin into its
//                     run's word -- the minimum is the same whatever order the lanes arrive in
//   k_replace_len     a lane a span: the heads store the bytes of their run's replacement, every other span 0
//   k_replace_check   a lane a document: raises ctl[kRepCtlGrow] for a document that reaches 4 GiB once replaced; lane 0 leaves the
//                     runs in ctl[kExcCtlExc] and the output's bytes in ctl[kExcCtlTotal].  The host reads the control block and
//                     refuses before anything is written
//   k_replace_place   a lane a span: a head stores its run's at, len, roff and the caller's run_new / run_len / run_rep, the last
//                     span of a run its delta; a lane a document: out_off and doc_run_off
//   k_replace_copy    from the OUTPUT side: a wave owns a tile of 4 KiB of the output, a lane a 16-byte chunk aligned to the output
//                     address.  A table of kRepLdsTable bytes or fewer goes into LDS once per workgroup, a larger one is read
//                     where it lies (it stays in L2).  One uniform binary search per tile over the plan, then a window of
//                     kRepWindow entries across the lanes, those that begin inside the tile with all their fields in LDS.
//                     A tile that no entry touches -- the entry in front has ended, the next begins behind the tile -- is a
//                     straight copy at one shift for every lane: no count, no LDS read.  In any other tile a chunk counts the
//                     entries in front of it with shuffles; a plain chunk (rep_chunk_plain) is one funnelled load and one store,
//                     like the tile above.  The chunks that meet entries are assembled segment by segment, and step k of the
//                     loop places the k-th segment of ALL FOUR trips' chunks of a lane: the wave runs as many steps as its
//                     busiest chunk has segments, not the sum of the four trips' busiest.  Bytes are stored singly only in
//                     the first and the last chunk of the range.
//
// Every launch reads only what an earlier launch stored.  The one atomic is k_replace_ids' minimum; the copy has none.  What a
// plan entry, a window and a chunk decide is in gft_replace_piece.hpp, which the host compiles too.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gft_replace.hpp"
#include "gft_wave_dev.hpp"

namespace gft {

namespace {

constexpr uint32_t kRepBlock = 256;         // 4 waves; the copy pass: a tile each

__global__ void __launch_bounds__(kExcTile) k_replace_ids(const ReplaceParams P) {
    const ExcerptParams& X = P.X;
    const uint64_t k = (uint64_t)blockIdx.x * kExcTile + threadIdx.x;
    if (X.ctl[kExcCtlDocs] || k >= X.n_spans) return;               // (offsets that descend: nothing behind them is read)
    const uint32_t id = rep_span_id(P.span_key, P.key_rep, P.n_keys, P.n_reps, X.s0 + k);
    if (id == kRepNoId) X.ctl[kRepCtlKey] = 1;                      // (refuses the call; the same value from every lane)
    else atomicMin(&P.rid[X.rank[k] + X.head[k] - 1], id);          // the run of span k: the heads up to and with it, less one
}

__global__ void __launch_bounds__(kExcTile) k_replace_len(const ReplaceParams P) {
    const ExcerptParams& X = P.X;
    const uint64_t k = (uint64_t)blockIdx.x * kExcTile + threadIdx.x;
    if (X.ctl[kExcCtlDocs] || k >= X.n_spans) return;
    uint32_t len = 0;
    if (X.head[k]) {
        const uint32_t id = P.rid[X.rank[k]];
        if (id < P.n_reps) len = (uint32_t)(P.rep_off[id + 1] - P.rep_off[id]);     // (no id: the call is refused behind the check)
    }
    P.pl[k] = len;
}

__global__ void __launch_bounds__(kExcTile) k_replace_check(const ReplaceParams P) {
    const ExcerptParams& X = P.X;
    const uint64_t d = (uint64_t)blockIdx.x * kExcTile + threadIdx.x;
    if (X.ctl[kExcCtlDocs]) return;
    if (d == 0) {
        X.ctl[kExcCtlExc] = X.rank[X.n_spans];
        X.ctl[kExcCtlTotal] = P.text_len - X.pos[X.n_spans] + P.ppos[X.n_spans];
    }
    if (d >= X.V.n_docs) return;
    const uint64_t a = X.V.span_off[d] - X.s0, b = X.V.span_off[d + 1] - X.s0;
    if (!rep_grow_ok(X.V.doc_off[d + 1] - X.V.doc_off[d], X.pos[b] - X.pos[a], P.ppos[b] - P.ppos[a])) X.ctl[kRepCtlGrow] = 1;
}

__global__ void __launch_bounds__(kExcTile) k_replace_place(const ReplaceParams P) {
    const ExcerptParams& X = P.X;
    const uint64_t k = (uint64_t)blockIdx.x * kExcTile + threadIdx.x;
    const uint64_t base = P.R.base;
    if (k < X.n_spans) {
        const uint32_t head = X.head[k];
        const uint64_t r = X.rank[k] + head - 1;
        if (head) {
            const uint64_t d = X.sdoc[k], ks = X.V.span_off[d] - X.s0;
            const uint64_t at = X.smin[k] - base + P.ppos[k] - X.pos[k];
            const uint32_t id = P.rid[r], len = P.pl[k];
            P.at[r] = at;
            P.len[r] = len;
            P.roff[r] = (uint32_t)P.rep_off[id];
            if (r < P.cap_runs) {
                if (P.run_new) P.run_new[r] = (uint32_t)(at - (X.V.doc_off[d] - base + P.ppos[ks] - X.pos[ks]));
                if (P.run_len) P.run_len[r] = len;
                if (P.run_rep) P.run_rep[r] = id;
            }
        }
        // behind the run's replacement the text goes on at the run's end: the shift is the bytes cut less the bytes put so far
        if (k + 1 == X.n_spans || X.head[k + 1]) P.delta[r] = base + X.pos[k + 1] - P.ppos[k + 1];
    }
    if (k <= X.V.n_docs && (P.out_off || P.doc_run_off)) {
        const uint64_t ks = X.V.span_off[k] - X.s0;
        if (P.doc_run_off) P.doc_run_off[k] = X.rank[ks];
        if (P.out_off) P.out_off[k] = X.V.doc_off[k] - base + P.ppos[ks] - X.pos[ks];
    }
}

// the window across the lanes as mark_lift reads it
struct WindowRel {
    uint32_t mine;
    __device__ __forceinline__ uint32_t operator()(uint32_t w) const { return (uint32_t)__shfl((int)mine, (int)w, 64); }
};

struct __attribute__((aligned(16))) U128 { uint64_t lo, hi; };

__global__ void __launch_bounds__(kRepBlock) k_replace_copy(const ReplaceParams P) {
    __shared__ U128 stab[(kRepLdsTable + kRepTableSlack) / 16];
    __shared__ uint32_t wrel[kRepBlock / 64][kRepWindow], wlen[kRepBlock / 64][kRepWindow], wroff[kRepBlock / 64][kRepWindow];
    __shared__ uint64_t wdelta[kRepBlock / 64][kRepWindow];
    const bool staged = P.tab_bytes <= kRepLdsTable;                // (the same in every lane of the grid)
    if (staged) {                                                   // the table's bytes and sixteen or more of the zeros behind them
        const uint32_t words = (P.tab_bytes + 15u) / 16u + 1u;
        for (uint32_t i = threadIdx.x; i < words; i += kRepBlock) stab[i] = reinterpret_cast<const U128*>(P.tab)[i];
    }
    const uint8_t* tab = staged ? reinterpret_cast<const uint8_t*>(stab) : P.tab;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wv = first_lane32(threadIdx.x >> 6);
    const uint64_t tile = (uint64_t)blockIdx.x * (kRepBlock / 64) + wv;
    const SelGeom G = P.G;
    const RepPlan R = P.R;
    const uint8_t* text = P.X.V.text;
    const bool live = tile < sel_tiles(G);                          // (the same in every lane of the wave)
    const uint64_t c0 = tile * (kSelTile / kSelChunk);
    uint64_t tile_lo = 0, tile_hi = 0, nb = 0;
    WindowRel win{0xFFFFFFFFu};
    RepEntry front{0, 0, 0, 0};
    if (live) {
        sel_chunk_range(G, c0, tile_lo, tile_hi);
        const uint64_t c_last = c0 + kSelTile / kSelChunk - 1;
        uint64_t l;
        sel_chunk_range(G, c_last, l, tile_hi);
        // the entries at or in front of the tile's first byte: uniform, searched on scalar values
        nb = first_lane64(rep_count(R, tile_lo));
        win.mine = rep_window_rel(R, nb, lane, tile_lo);
        front = nb ? rep_entry(R, nb - 1) : rep_entry_none(R);
        front = RepEntry{first_lane64(front.at), first_lane64(front.delta), first_lane32(front.len), first_lane32(front.roff)};
    }
    const uint32_t span = (uint32_t)(tile_hi - tile_lo);
    wrel[wv][lane] = win.mine;
    if (win.mine < span) {                                          // (an entry that begins inside the tile: what a chunk may ask for)
        wdelta[wv][lane] = R.delta[nb + lane];
        wlen[wv][lane] = R.len[nb + lane];
        wroff[wv][lane] = R.roff[nb + lane];
    }
    __syncthreads();                                                // (every wave of the workgroup, the ones past the range too)
    if (!live) return;
    const RepWin W{wrel[wv], wdelta[wv], wlen[wv], wroff[wv], nb, tile_lo, span, front};
    // no entry touches the tile: the one in front has ended, the next begins behind the tile's last byte
    const bool easy = front.at + front.len <= tile_lo && first_lane32(win.mine) >= span;
    uint64_t lo[kSelTrips], hi[kSelTrips];
    RepCursor cur[kSelTrips];
    SelV acc[kSelTrips];
#pragma unroll
    for (uint32_t t = 0; t < kSelTrips; t++) {
        const uint64_t c = c0 + t * 64u + lane;
        sel_chunk_range(G, c, lo[t], hi[t]);
        const bool valid = lo[t] < hi[t];
        const uint32_t j = sel_chunk_byte(G, c, lo[t]);
        acc[t] = SelV{0, 0};
        cur[t] = RepCursor{hi[t], 0, 0};                            // (nothing left to assemble)
        if (easy) {
            if (valid) acc[t] = sel_shift(sel_load(text + (front.delta + lo[t]), (uint32_t)(hi[t] - lo[t])), j);
            continue;
        }
        const uint32_t lo_rel = valid ? (uint32_t)(lo[t] - tile_lo) : 0u, hi_rel = valid ? (uint32_t)(hi[t] - tile_lo) : 0u;
        const uint32_t cnt = mark_lift(win, lo_rel);
        const uint32_t next_rel = win(cnt);                         // (every lane makes the call)
        if (!valid) continue;
        if (cnt < kRepWindow - 1) {
            const RepEntry E = cnt ? RepEntry{tile_lo + wrel[wv][cnt - 1], wdelta[wv][cnt - 1], wlen[wv][cnt - 1], wroff[wv][cnt - 1]} : front;
            if (rep_chunk_plain(E, lo[t], next_rel, hi_rel)) acc[t] = sel_shift(sel_load(text + (E.delta + lo[t]), (uint32_t)(hi[t] - lo[t])), j);
            else cur[t] = RepCursor{lo[t], nb + cnt, j};
        } else {                                                    // (the window does not say: this lane searches the plan)
            cur[t] = RepCursor{lo[t], rep_count(R, lo[t]), j};
        }
    }
    // step k: the k-th segment of each of the lane's four chunks
    for (;;) {
        bool more = false;
#pragma unroll
        for (uint32_t t = 0; t < kSelTrips; t++) {
            if (cur[t].p < hi[t]) {
                rep_segment(R, W, text, tab, hi[t], cur[t], acc[t]);
                more |= cur[t].p < hi[t];
            }
        }
        if (!more) break;
    }
#pragma unroll
    for (uint32_t t = 0; t < kSelTrips; t++) {
        const uint64_t c = c0 + t * 64u + lane;
        if (lo[t] < hi[t]) sel_store(P.out, G, c, lo[t], hi[t], acc[t]);
    }
}

unsigned blocks_for(uint64_t n) { return (unsigned)std::max<uint64_t>((n + kExcTile - 1) / kExcTile, 1); }

}  // namespace

hipError_t launch_replace_ids(const ReplaceParams& P, hipStream_t st) {
    if (!P.X.n_spans) return hipSuccess;
    k_replace_ids<<<dim3(blocks_for(P.X.n_spans)), dim3(kExcTile), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_replace_len(const ReplaceParams& P, hipStream_t st) {
    if (!P.X.n_spans) return hipSuccess;
    k_replace_len<<<dim3(blocks_for(P.X.n_spans)), dim3(kExcTile), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_replace_check(const ReplaceParams& P, hipStream_t st) {
    if (!P.X.V.n_docs) return hipSuccess;
    k_replace_check<<<dim3(blocks_for(P.X.V.n_docs)), dim3(kExcTile), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_replace_place(const ReplaceParams& P, hipStream_t st) {
    if (!P.X.V.n_docs) return hipSuccess;
    k_replace_place<<<dim3(blocks_for(std::max(P.X.n_spans, P.X.V.n_docs + 1))), dim3(kExcTile), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_replace_copy(const ReplaceParams& P, hipStream_t st) {
    const uint64_t tiles = sel_tiles(P.G);
    if (!tiles) return hipSuccess;
    k_replace_copy<<<dim3((unsigned)((tiles + kRepBlock / 64 - 1) / (kRepBlock / 64))), dim3(kRepBlock), 0, st>>>(P);
    return hipGetLastError();
}

}  // namespace gft
