// gft_split.hip -- a resident blob cut into line documents (gft_split_lines_device), gfx950 / wave64.
//
//   (blob, len)  ->  doc_off [n + 1]: where every document starts, and len
//
//   k_split_count   a wave owns a tile of 4 KiB and reads it in four trips of 1 KiB, a lane 16 bytes of a trip (the four loads
//                   are issued together).  AFTER_NL: newlines per tile -> cnt.  JSON_LINES: the tile's SplitSum -> sums
//   k_split_carry   JSON_LINES only, ONE workgroup: walks the tile summaries in trips of 1024 (a thread four consecutive tiles),
//                   keeps the carry from trip to trip and leaves for every tile the carry in front of it and its count with
//                   the document its head starts -> carry, cnt.  Linear in the tiles, whatever the lines' lengths.
//   (k_scan_* of gft_kernels.hip: cnt -> base)
//   k_split_write   the count pass's walk again; every lane stores the starts of its piece at base[tile] + the prefix over the
//                   wave (DPP), carried from trip to trip
//
// Every launch reads only what an earlier launch stored: no workgroup waits for another, no flag is polled, no atomic is used,
// and the offsets come out ascending whatever the schedule.  What a piece, a trip and a tile say is decided by
// gft_split_piece.hpp, which the host compiles too.  Memory bound: two reads of the text.
#include <hip/hip_runtime.h>

#include "gft_kernels.hpp"
#include "gft_split.hpp"
#include "gft_wave_dev.hpp"

namespace gft {

namespace {

constexpr uint32_t kSplitBlock = 256;       // 4 waves, a tile each

// the wave's tile: its four trips' pieces in registers (w[t]: the piece at o[t], n[t] of its bytes in the blob)
struct TilePieces {
    uint32_t w[kSplitTrips][4];
    uint64_t o[kSplitTrips];
    uint32_t n[kSplitTrips];
};
__device__ __forceinline__ void load_tile(const uint8_t* __restrict__ blob, uint64_t len, uint64_t tile, uint32_t lane, TilePieces& T) {
#pragma unroll
    for (uint32_t t = 0; t < kSplitTrips; t++) {
        T.o[t] = tile * kSplitTile + t * kSplitTrip + lane * kSplitPiece;
        T.n[t] = T.o[t] < len ? (uint32_t)(len - T.o[t] < kSplitPiece ? len - T.o[t] : kSplitPiece) : 0u;
        T.w[t][0] = T.w[t][1] = T.w[t][2] = T.w[t][3] = 0;
        if (T.n[t]) split_load_piece(blob + T.o[t], T.n[t], T.w[t]);
    }
}

// one trip of GFT_SPLIT_JSON_LINES in a wave: the lanes' flags as masks
struct TripMasks {
    uint64_t NL, HEAD, TAIL;
};
__device__ __forceinline__ TripMasks trip_masks(uint32_t flags) {
    return TripMasks{__ballot((flags & kSplitHasNl) != 0), __ballot((flags & kSplitHead) != 0), __ballot((flags & kSplitTail) != 0)};
}

template <int MODE>
__global__ void __launch_bounds__(kSplitBlock) k_split_count(const SplitParams P) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t tile = ((uint64_t)blockIdx.x * kSplitBlock + threadIdx.x) >> 6;
    if (tile >= P.n_tiles) return;                                       // (the same in every lane)
    TilePieces T;
    load_tile(P.blob, P.len, tile, lane, T);
    if (MODE == GFT_SPLIT_AFTER_NL) {
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t t = 0; t < kSplitTrips; t++) {
            uint32_t nl, nw;
            split_piece_masks(T.w[t], split_nl_bytes(T.o[t], P.len), nl, nw);
            sum += (uint32_t)__builtin_popcount(nl);
        }
        sum = wave_incl_scan(sum);
        if (lane == 63) P.cnt[tile] = sum;
        return;
    }
    SplitSum S{0, 0, 0};
#pragma unroll
    for (uint32_t t = 0; t < kSplitTrips; t++) {
        uint32_t nl, nw;
        split_piece_masks(T.w[t], T.n[t], nl, nw);
        const uint32_t flags = split_piece_flags(nl, nw);
        const TripMasks M = trip_masks(flags);
        const SplitFrom F = split_lane_prefix(M.NL, M.HEAD, M.TAIL, lane, 0);
        // (a head with no newline of the trip in front of it belongs to the trip's head: the carry decides it)
        const bool bnd = F.src >= 0 && (flags & kSplitHead) && !F.open;
        const uint32_t inner = wave_incl_scan((uint32_t)__builtin_popcount(split_inner_events(nl, nw)));
        int last;
        SplitSum trip;
        trip.flags = split_wave_flags(M.NL, M.HEAD, M.TAIL, &last);
        trip.count = lane_value(inner, 63) + (uint32_t)__builtin_popcountll(__ballot(bnd));
        const uint32_t last_bit = nl ? 31u - (uint32_t)__builtin_clz(nl) : 0u;
        trip.last_nl = last >= 0 ? tile * kSplitTile + t * kSplitTrip + (uint32_t)last * kSplitPiece + lane_value(last_bit, last) : 0;
        S = split_combine(S, trip);
    }
    if (lane == 0) P.sums[tile] = S;
}

// ONE workgroup.  A thread combines its four tiles; the threads of a wave resolve each other with three ballots, the waves
// through LDS; the carry behind a trip is the next one's.
__global__ void __launch_bounds__(kSplitCarryBlock) k_split_carry(const SplitParams P) {
    __shared__ SplitSum wave_sum[2][kSplitCarryBlock / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    SplitCarry carry{0, 0, 0};                                            // in front of the blob: a blank line that starts at 0
    uint32_t buf = 0;
    for (uint64_t t0 = 0; t0 < P.n_tiles; t0 += kSplitCarryTrip, buf ^= 1u) {
        const uint64_t first = t0 + (uint64_t)threadIdx.x * kSplitCarryRun;
        SplitSum s[kSplitCarryRun], run{0, 0, 0};
#pragma unroll
        for (uint32_t i = 0; i < kSplitCarryRun; i++) {
            s[i] = first + i < P.n_tiles ? P.sums[first + i] : SplitSum{0, 0, 0};
            run = split_combine(run, s[i]);
        }
        const TripMasks M = trip_masks(run.flags);
        int last;
        SplitSum ws;
        ws.flags = split_wave_flags(M.NL, M.HEAD, M.TAIL, &last);
        ws.count = 0;
        ws.last_nl = last >= 0 ? lane_value64(run.last_nl, last) : 0;
        if (lane == 0) wave_sum[buf][wave] = ws;
        __syncthreads();                                                  // (two buffers: one barrier per trip)
        SplitCarry c = carry;
        for (uint32_t v = 0; v < kSplitCarryBlock / 64; v++) {
            if (v == wave) c = carry;
            carry = split_advance(carry, wave_sum[buf][v]);
        }
        // c: in front of this wave's runs; mine: in front of this thread's
        const SplitFrom F = split_lane_prefix(M.NL, M.HEAD, M.TAIL, lane, c.open);
        const uint64_t from = shuffle64(run.last_nl, F.src >= 0 ? F.src : 0);
        SplitCarry mine{F.src >= 0 ? from + 1 : c.line_start, F.open, 0};
#pragma unroll
        for (uint32_t i = 0; i < kSplitCarryRun; i++) {
            if (first + i < P.n_tiles) {
                P.carry[first + i] = mine;
                P.cnt[first + i] = s[i].count + split_boundary(mine, s[i]);
            }
            mine = split_advance(mine, s[i]);
        }
    }
}

template <int MODE>
__global__ void __launch_bounds__(kSplitBlock) k_split_write(const SplitParams P) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t tile = ((uint64_t)blockIdx.x * kSplitBlock + threadIdx.x) >> 6;
    if (tile >= P.n_tiles) return;
    TilePieces T;
    load_tile(P.blob, P.len, tile, lane, T);
    // document 0 starts at 0; document n ends at len (rank 0 is nobody's event: AFTER_NL counts from 1, JSON_LINES skips it)
    uint64_t k = P.base[tile] + (MODE == GFT_SPLIT_AFTER_NL ? 1u : 0u);
    if (lane == 0) {
        if (tile == 0 && P.cap) P.out[0] = 0;
        if (tile == P.n_tiles - 1) {
            const uint64_t n = P.base[P.n_tiles] + (MODE == GFT_SPLIT_AFTER_NL ? 1u : 0u);
            if (n && n < P.cap) P.out[n] = P.len;
        }
    }
    if (MODE == GFT_SPLIT_AFTER_NL) {
#pragma unroll
        for (uint32_t t = 0; t < kSplitTrips; t++) {
            uint32_t nl, nw;
            split_piece_masks(T.w[t], split_nl_bytes(T.o[t], P.len), nl, nw);
            const uint32_t c = (uint32_t)__builtin_popcount(nl), incl = wave_incl_scan(c);
            split_emit_after_nl(nl, T.o[t], k + (incl - c), P.out, P.cap);
            k += lane_value(incl, 63);
        }
        return;
    }
    SplitCarry carry = P.carry[tile];
#pragma unroll
    for (uint32_t t = 0; t < kSplitTrips; t++) {
        uint32_t nl, nw;
        split_piece_masks(T.w[t], T.n[t], nl, nw);
        const uint32_t flags = split_piece_flags(nl, nw);
        const TripMasks M = trip_masks(flags);
        const SplitFrom F = split_lane_prefix(M.NL, M.HEAD, M.TAIL, lane, carry.open);
        const uint32_t last_bit = nl ? 31u - (uint32_t)__builtin_clz(nl) : 0u;
        const uint64_t my_last = T.o[t] + last_bit;                       // (read only from lanes that have a newline)
        const uint64_t from = shuffle64(my_last, F.src >= 0 ? F.src : 0);
        const uint64_t line_start = F.src >= 0 ? from + 1 : carry.line_start;
        uint32_t ev = split_inner_events(nl, nw);
        if ((flags & kSplitHead) && !F.open) ev |= nw & (0u - nw);        // the head's first byte starts a document
        const uint32_t c = (uint32_t)__builtin_popcount(ev), incl = wave_incl_scan(c);
        split_emit_lines(ev, nl, T.o[t], line_start, k + (incl - c), P.out, P.cap);
        k += lane_value(incl, 63);
        int last;
        SplitSum trip;
        trip.flags = split_wave_flags(M.NL, M.HEAD, M.TAIL, &last);
        trip.count = 0;
        trip.last_nl = last >= 0 ? lane_value64(my_last, last) : 0;
        carry = split_advance(carry, trip);
    }
}

unsigned split_grid(uint64_t n_tiles) { return (unsigned)((n_tiles + kSplitBlock / 64 - 1) / (kSplitBlock / 64)); }

}  // namespace

hipError_t launch_split_count(const SplitParams& P, uint32_t mode, hipStream_t st) {
    if (!P.n_tiles) return hipSuccess;
    if (mode == GFT_SPLIT_AFTER_NL) k_split_count<GFT_SPLIT_AFTER_NL><<<dim3(split_grid(P.n_tiles)), dim3(kSplitBlock), 0, st>>>(P);
    else k_split_count<GFT_SPLIT_JSON_LINES><<<dim3(split_grid(P.n_tiles)), dim3(kSplitBlock), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_split_carry(const SplitParams& P, hipStream_t st) {
    if (!P.n_tiles) return hipSuccess;
    k_split_carry<<<dim3(1), dim3(kSplitCarryBlock), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_split_write(const SplitParams& P, uint32_t mode, hipStream_t st) {
    if (!P.n_tiles) return hipSuccess;
    if (mode == GFT_SPLIT_AFTER_NL) k_split_write<GFT_SPLIT_AFTER_NL><<<dim3(split_grid(P.n_tiles)), dim3(kSplitBlock), 0, st>>>(P);
    else k_split_write<GFT_SPLIT_JSON_LINES><<<dim3(split_grid(P.n_tiles)), dim3(kSplitBlock), 0, st>>>(P);
    return hipGetLastError();
}

}  // namespace gft
