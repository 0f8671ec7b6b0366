// gft_context.hip -- context lines round the documents that matched (gft_context_docs_device), gfx950 / wave64.
//
//   (sel[] of k_select_mark, fence[], before, after)  ->  keep[d], len[d], newgroup[d]; the compact arrays of the select's copy pass
//
//   k_ctx_reach          a wave a tile of 64 consecutive documents: two ballots give the tile's selected word and its fence word;
//                        lane 0 stores them and what they say to the other tiles (last / first selected, last / first fence)
//   k_ctx_carry_blocks   a wave a carry block of 64 tiles, a lane a tile: the block's own four extrema and its selected count
//   k_ctx_carry_spine    ONE wave over the blocks, 64 per trip: the maxima forward, the minima backward, exclusive, in place; the
//                        selected count of the batch -> ctl[kCtxCtlHits]
//   k_ctx_carry_tiles    a wave a carry block again: the exclusive extrema inside the block joined with the block's -> carry[t]
//   k_ctx_decide         a wave a tile again: every lane finds its nearest selected document on either side that no fence separates
//                        (clz / ctz on the masked words inside the tile, the carry outside) -> keep, len, newgroup; the left
//                        neighbour's answer comes from the wave's ballot, for lane 0 from the tile's own carry
//   (k_scan_* of gft_kernels.hip: len -> pos, keep -> rank, newgroup -> grank; k_ctx_pack gathers what the host reads back)
//   k_ctx_place          a thread a document: c_off / c_src (complete), out_off / doc_idx / kind and group_off (capped)
//   (k_select_copy of gft_select.hip, unchanged, for the bytes)
//
// Every launch reads only what an earlier launch stored; no workgroup waits for another; no atomics.  What a tile, a lane and a
// carry decide is gft_context_piece.hpp, which the host compiles too.  Traffic: the flags and three prefix sums per document, a few
// words per tile -- beside the copy of the kept bytes.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gft_context.hpp"
#include "gft_wave_dev.hpp"

namespace gft {

namespace {

constexpr uint32_t kCtxBlock = 256;         // 4 waves, each on a tile (or a carry block) of its own: no LDS, no barrier

// over the lanes of a wave: the maximum / minimum of the lanes in front of / behind this one (exclusive), and of all in `all`
__device__ __forceinline__ uint64_t wave_max_front(uint64_t v, uint32_t lane, uint64_t& all) {
    uint64_t incl = v;
#pragma unroll
    for (uint32_t s = 1; s < 64; s <<= 1) {
        const uint64_t o = up64(incl, s);
        if (lane >= s) incl = ctx_max(incl, o);
    }
    all = lane_value64(incl, 63);
    const uint64_t ex = up64(incl, 1);
    return lane ? ex : 0;
}
__device__ __forceinline__ uint64_t wave_min_behind(uint64_t v, uint32_t lane, uint64_t& all) {
    uint64_t incl = v;
#pragma unroll
    for (uint32_t s = 1; s < 64; s <<= 1) {
        const uint64_t o = down64(incl, s);
        if (lane + s < 64) incl = ctx_min(incl, o);
    }
    all = lane_value64(incl, 0);
    const uint64_t ex = down64(incl, 1);
    return lane < 63 ? ex : kCtxNone;
}

__global__ void __launch_bounds__(kCtxBlock) k_ctx_reach(const ContextParams P) {
    const WaveId w(kCtxBlock);
    for (uint64_t t = w.wave; t < P.n_tiles; t += w.n_waves) {
        const uint64_t base = t * kCtxTile, d = base + w.lane;
        const bool in = d < P.n_docs;
        const uint64_t S = __ballot(in && P.sel[d] != 0);
        const uint64_t F = __ballot(in && P.fence && P.fence[d] != 0);
        if (w.lane == 0) {
            P.word_sel[t] = S;
            P.word_fence[t] = F;
            P.sum[t] = ctx_last(S, base);
            P.sum[P.n_tiles + t] = ctx_last(F, base);
            P.sum[2 * P.n_tiles + t] = ctx_first(S, base);
            P.sum[3 * P.n_tiles + t] = ctx_first(F, base);
        }
    }
}

__global__ void __launch_bounds__(kCtxBlock) k_ctx_carry_blocks(const ContextParams P) {
    const WaveId w(kCtxBlock);
    for (uint64_t b = w.wave; b < P.n_blocks; b += w.n_waves) {
        const uint64_t t = b * kCtxCarry + w.lane;
        const bool in = t < P.n_tiles;
        uint64_t all[4];
        (void)wave_max_front(in ? P.sum[t] : 0, w.lane, all[0]);
        (void)wave_max_front(in ? P.sum[P.n_tiles + t] : 0, w.lane, all[1]);
        (void)wave_min_behind(in ? P.sum[2 * P.n_tiles + t] : kCtxNone, w.lane, all[2]);
        (void)wave_min_behind(in ? P.sum[3 * P.n_tiles + t] : kCtxNone, w.lane, all[3]);
        // the block's selected documents: the popcounts summed over the lanes
        uint64_t cnt = in ? (uint64_t)__popcll(P.word_sel[t]) : 0;
#pragma unroll
        for (uint32_t s = 32; s; s >>= 1) cnt += down64(cnt, s);
        if (w.lane == 0) {
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) P.part[k * P.n_blocks + b] = all[k];
            P.part[4 * P.n_blocks + b] = cnt;
        }
    }
}

// one wave
__global__ void __launch_bounds__(kCtxSpine) k_ctx_carry_spine(const ContextParams P) {
    const uint32_t lane = threadIdx.x;
    static_assert(kCtxSpine == 64 && kCtxCarry == 64 && kCtxTile == 64, "a tile, a carry block and a trip of the spine are a wave");
    const uint64_t n = P.n_blocks, trips = (n + 63) / 64;
    uint64_t* ps = P.part;
    uint64_t* pf = P.part + n;
    uint64_t* ns = P.part + 2 * n;
    uint64_t* nf = P.part + 3 * n;
    // (a trip's values are requested a trip ahead, in front of the stores of the trip at hand: the one wave waits for memory once,
    // not once per trip)
    uint64_t cs = 0, cf = 0, hits = 0;
    uint64_t vs = lane < n ? ps[lane] : 0, vf = lane < n ? pf[lane] : 0, vh = lane < n ? P.part[4 * n + lane] : 0;
    for (uint64_t k = 0; k < trips; k++) {
        const uint64_t b = k * 64 + lane, b1 = b + 64;
        const bool in1 = b1 < n;
        const uint64_t ws = in1 ? ps[b1] : 0, wf = in1 ? pf[b1] : 0, wh = in1 ? P.part[4 * n + b1] : 0;
        uint64_t as, af;
        const uint64_t es = wave_max_front(vs, lane, as), ef = wave_max_front(vf, lane, af);
        hits += vh;
        if (b < n) { ps[b] = ctx_max(cs, es); pf[b] = ctx_max(cf, ef); }
        cs = ctx_max(cs, as); cf = ctx_max(cf, af);
        vs = ws; vf = wf; vh = wh;
    }
    cs = kCtxNone; cf = kCtxNone;
    {
        const uint64_t b = (trips - 1) * 64 + lane;
        vs = b < n ? ns[b] : kCtxNone; vf = b < n ? nf[b] : kCtxNone;
    }
    for (uint64_t k = trips; k-- > 0;) {
        const uint64_t b = k * 64 + lane;
        const bool in1 = k > 0;                                    // (the trip in front is a full one)
        const uint64_t ws = in1 ? ns[b - 64] : kCtxNone, wf = in1 ? nf[b - 64] : kCtxNone;
        uint64_t as, af;
        const uint64_t es = wave_min_behind(vs, lane, as), ef = wave_min_behind(vf, lane, af);
        if (b < n) { ns[b] = ctx_min(cs, es); nf[b] = ctx_min(cf, ef); }
        cs = ctx_min(cs, as); cf = ctx_min(cf, af);
        vs = ws; vf = wf;
    }
#pragma unroll
    for (uint32_t s = 32; s; s >>= 1) hits += down64(hits, s);
    if (lane == 0) P.ctl[kCtxCtlHits] = hits;
}

__global__ void __launch_bounds__(kCtxBlock) k_ctx_carry_tiles(const ContextParams P) {
    const WaveId w(kCtxBlock);
    for (uint64_t b = w.wave; b < P.n_blocks; b += w.n_waves) {
        const uint64_t t = b * kCtxCarry + w.lane;
        const bool in = t < P.n_tiles;
        uint64_t all;
        const uint64_t e0 = wave_max_front(in ? P.sum[t] : 0, w.lane, all);
        const uint64_t e1 = wave_max_front(in ? P.sum[P.n_tiles + t] : 0, w.lane, all);
        const uint64_t e2 = wave_min_behind(in ? P.sum[2 * P.n_tiles + t] : kCtxNone, w.lane, all);
        const uint64_t e3 = wave_min_behind(in ? P.sum[3 * P.n_tiles + t] : kCtxNone, w.lane, all);
        if (in) {
            P.carry[t] = ctx_max(e0, P.part[b]);
            P.carry[P.n_tiles + t] = ctx_max(e1, P.part[P.n_blocks + b]);
            P.carry[2 * P.n_tiles + t] = ctx_min(e2, P.part[2 * P.n_blocks + b]);
            P.carry[3 * P.n_tiles + t] = ctx_min(e3, P.part[3 * P.n_blocks + b]);
        }
    }
}

__global__ void __launch_bounds__(kCtxBlock) k_ctx_decide(const ContextParams P) {
    const WaveId w(kCtxBlock);
    for (uint64_t t = w.wave; t < P.n_tiles; t += w.n_waves) {
        const uint64_t base = t * kCtxTile, d = base + w.lane;
        // (the same in every lane: scalar values)
        const uint64_t S = first_lane64(P.word_sel[t]), F = first_lane64(P.word_fence[t]);
        const CtxCarry c{first_lane64(P.carry[t]), first_lane64(P.carry[P.n_tiles + t]), first_lane64(P.carry[2 * P.n_tiles + t]),
                         first_lane64(P.carry[3 * P.n_tiles + t])};
        const bool in = d < P.n_docs;
        const uint32_t keep = in ? ctx_keep(S, F, c, base, w.lane, P.before, P.after) : 0u;
        const uint64_t K = __ballot(keep != 0);
        const uint32_t left = w.lane ? (uint32_t)(K >> (w.lane - 1)) & 1u : (base ? ctx_keep_left(S, F, c, base, P.before, P.after) : 0u);
        if (in) {
            const uint64_t a = P.doc_off[d], b = P.doc_off[d + 1];
            P.keep[d] = keep;
            P.len[d] = (keep && sel_doc_ok(a, b)) ? (uint32_t)(b - a) : 0u;
            P.newgroup[d] = ctx_new_group(keep, left, d, (uint32_t)(F >> w.lane) & 1u);
        }
    }
}

__global__ void k_ctx_pack(const ContextParams P) {
    P.ctl[kSelCtlTotal] = P.pos[P.n_docs];
    P.ctl[kSelCtlM] = P.rank[P.n_docs];
    P.ctl[kSelCtlLo] = P.doc_off[0];
    P.ctl[kSelCtlHi] = P.doc_off[P.n_docs];
    P.ctl[kCtxCtlGroups] = P.grank[P.n_docs];
}

__global__ void __launch_bounds__(kCtxBlock) k_ctx_place(const ContextParams P) {
    const uint64_t d = (uint64_t)blockIdx.x * kCtxBlock + threadIdx.x;
    if (d == 0) {
        sel_place_close(P, P.m, P.total);
        if (P.group_off && P.groups <= P.cap_groups) P.group_off[P.groups] = P.m;
    }
    uint64_t r;
    if (d >= P.n_docs || !sel_place_doc(P, d, r)) return;
    if (r < P.cap_docs) P.kind[r] = (uint8_t)((P.word_sel[d / kCtxTile] >> (d % kCtxTile)) & 1u);
    const uint64_t g = P.grank[d];
    if (P.grank[d + 1] != g && P.group_off && g <= P.cap_groups) P.group_off[g] = r;
}

}  // namespace

hipError_t launch_context_reach(const ContextParams& P, unsigned n_cus, hipStream_t st) {
    if (!P.n_docs) return hipSuccess;
    k_ctx_reach<<<dim3(wave_grid(P.n_tiles, kCtxBlock, n_cus)), dim3(kCtxBlock), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_context_carry(const ContextParams& P, unsigned n_cus, hipStream_t st) {
    if (!P.n_docs) return hipSuccess;
    k_ctx_carry_blocks<<<dim3(wave_grid(P.n_blocks, kCtxBlock, n_cus)), dim3(kCtxBlock), 0, st>>>(P);
    k_ctx_carry_spine<<<dim3(1), dim3(kCtxSpine), 0, st>>>(P);
    k_ctx_carry_tiles<<<dim3(wave_grid(P.n_blocks, kCtxBlock, n_cus)), dim3(kCtxBlock), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_context_decide(const ContextParams& P, unsigned n_cus, hipStream_t st) {
    if (!P.n_docs) return hipSuccess;
    k_ctx_decide<<<dim3(wave_grid(P.n_tiles, kCtxBlock, n_cus)), dim3(kCtxBlock), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_context_pack(const ContextParams& P, hipStream_t st) {
    k_ctx_pack<<<dim3(1), dim3(1), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_context_place(const ContextParams& P, hipStream_t st) {
    // (one block at least: thread 0 closes c_off, out_off and group_off)
    k_ctx_place<<<dim3((unsigned)std::max<uint64_t>((P.n_docs + kCtxBlock - 1) / kCtxBlock, 1)), dim3(kCtxBlock), 0, st>>>(P);
    return hipGetLastError();
}

}  // namespace gft
