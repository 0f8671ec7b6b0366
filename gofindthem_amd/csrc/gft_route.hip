// gft_route.hip -- documents routed to per-bucket runs of one blob (gft_route_docs_device), gfx950 / wave64.
//
//   (text, doc_off, hit rows, n_buckets masks, mode, rest, also)  ->  out: the entries' documents back to back, bucket by bucket
//   and in input order inside a bucket, out_off, doc_idx; the bucket borders in entries and in bytes
//
//   k_route_mark    reads the rows with join_bit_rows of gft_bitrows_dev.hpp, as k_select_mark does (64 / W' rows per wave for
//                   W <= 64, a row per wave in steps of 64 words above that).  A lane compares its word with the same word of
//                   every mask -- the masks lie in LDS for W <= 64 (at most 64 x 64 words, 16 KB; lanes on consecutive words: no
//                   bank conflict), and come through L2 above that -- and the 64-bit hit words are joined over the row by xor shuffles
//                   -> member[d] (bit b: an entry in bucket b), len[d]; raises ctl[kRouteCtlFlag] as the select's mark pass does
//   k_route_count   a wave a tile of 64 documents, lane b owns bucket b: per bucket one ballot of bit b and a popcount
//                   -> cnt[b * n_tiles + tile]; tile_bytes[tile] (the lengths once per entry, joined by shuffles)
//   (k_scan_* of gft_kernels.hip: cnt -> base, B * n_tiles entries in one pass: every (bucket, tile) base, the borders, m)
//   k_route_pack    one block: m, the B + 1 bucket borders, the sum of tile_bytes, doc_off[0], doc_off[n] -> ctl
//   k_route_place   the same ballots per tile: rank = base[b * n_tiles + tile] + popcount(ballot & lanes below)
//                   -> ent_len[r], c_src[r], doc_idx[r] (capped).  The bucket loop is uniform across the wave
//   (k_scan_*: ent_len -> c_off, m entries: where every entry starts in the output, in 64 bits)
//   k_route_finish  out_off = the capped prefix of c_off; block 0 gathers bucket_byte[b] = c_off[bucket_doc[b]] into ctl
//   (k_select_copy of gft_select.hip writes the blob from c_off / c_src: it does not care in which order the entries come)
//
// Every launch reads only what an earlier launch stored; no atomics; the flag is raised with a plain store.  What a word, a
// member word and a rank are is decided by gft_route_piece.hpp, which the host compiles too.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gft_bitrows_dev.hpp"
#include "gft_kernels.hpp"
#include "gft_route.hpp"

namespace gft {

namespace {

constexpr uint32_t kRouteBlock = kBitRowsBlock;         // 4 waves
constexpr uint32_t kRouteLdsWords = 64 * 64;            // the masks of W <= 64: GFT_ROUTE_MAX_BUCKETS rows of at most 64 words

// What join_bit_rows joins over a row: the 64-bit word of the masks the row's words meet.  Masks: where the masks lie -- the
// kernel's LDS array itself for W <= 64 (so that the inlined walk reads it as LDS), the engine's copy above that.
template <class Masks>
struct RouteSink {
    using Value = uint64_t;
    using Col = uint32_t;
    const RouteParams& P;
    Masks masks;
    __device__ __forceinline__ uint64_t identity() const { return 0; }
    __device__ __forceinline__ uint32_t column(uint32_t j) const { return j; }
    __device__ __forceinline__ uint64_t word(uint32_t w, uint32_t j) const {
        uint64_t hits = 0;
        if (w)
            for (uint32_t k = 0; k < P.n_buckets; k++) hits |= route_word_bit(w, masks[(uint64_t)k * P.W + j], k);
        return hits;
    }
    __device__ __forceinline__ uint64_t join(uint64_t a, uint64_t b) const { return a | b; }
    __device__ __forceinline__ uint64_t exchange(uint64_t v, uint32_t s) const { return shuffle_xor64(v, (int)s); }
    __device__ __forceinline__ void finish(uint64_t row, uint64_t hits) const {
        const uint64_t a = P.doc_off[row], b = P.doc_off[row + 1];
        const uint32_t ok = sel_doc_ok(a, b);
        if (!ok) P.ctl[kRouteCtlFlag] = 1;
        P.len[row] = ok ? (uint32_t)(b - a) : 0u;
        P.member[row] = route_member(hits, P.n_buckets, P.mode, P.rest, (P.also && P.also[row]) ? 1u : 0u);
    }
};

__global__ void __launch_bounds__(kRouteBlock) k_route_mark(const RouteParams P) {
    __shared__ uint32_t s_masks[kRouteLdsWords];
    const BitRows B{P.bitmap, P.n_docs, P.W, P.lg, 0};
    if (P.W == 0 || P.n_buckets == 0) {
        const RouteSink<const uint32_t*> S{P, P.masks};
        const uint64_t thread = (uint64_t)blockIdx.x * kRouteBlock + threadIdx.x, n_threads = (uint64_t)gridDim.x * kRouteBlock;
        for (uint64_t row = thread; row < P.n_docs; row += n_threads) S.finish(row, 0);
    } else if (P.W <= 64) {
        for (uint32_t i = threadIdx.x; i < P.n_buckets * P.W; i += kRouteBlock) s_masks[i] = P.masks[i];
        __syncthreads();
        join_bit_rows(B, RouteSink<const uint32_t (&)[kRouteLdsWords]>{P, s_masks});
    } else {
        join_bit_rows(B, RouteSink<const uint32_t*>{P, P.masks});
    }
}

__global__ void __launch_bounds__(kRouteBlock) k_route_count(const RouteParams P) {
    const WaveId w(kRouteBlock);
    const uint32_t lane = w.lane;
    for (uint64_t tile = w.wave; tile < P.n_tiles; tile += w.n_waves) {
        const uint64_t d = tile * kRouteTileDocs + lane;
        const uint64_t mem = d < P.n_docs ? P.member[d] : 0ull;
        uint64_t bytes = d < P.n_docs ? route_doc_bytes(P.len[d], mem) : 0ull;
        uint32_t mine = 0;
        for (uint32_t b = 0; b < P.B; b++) {                        // (uniform)
            const uint32_t c = route_popcount(__ballot((mem >> b) & 1ull));
            if (lane == b) mine = c;
        }
        if (lane < P.B) P.cnt[route_cell(lane, P.n_tiles, tile)] = mine;
        for (uint32_t s = 1; s < 64; s <<= 1) bytes += shuffle_xor64(bytes, (int)s);
        if (lane == 0) P.tile_bytes[tile] = bytes;
    }
}

__global__ void __launch_bounds__(kRouteBlock) k_route_pack(const RouteParams P) {
    __shared__ uint64_t s_sum[kRouteBlock];
    uint64_t sum = 0;
    for (uint64_t t = threadIdx.x; t < P.n_tiles; t += kRouteBlock) sum += P.tile_bytes[t];
    s_sum[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t s = kRouteBlock / 2; s; s >>= 1) {
        if (threadIdx.x < s) s_sum[threadIdx.x] += s_sum[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x <= P.B) P.ctl[kRouteCtlDoc + threadIdx.x] = P.base[route_cell(threadIdx.x, P.n_tiles, 0)];
    if (threadIdx.x == 0) {
        P.ctl[kRouteCtlM] = P.base[route_cell(P.B, P.n_tiles, 0)];
        P.ctl[kRouteCtlTotal] = s_sum[0];
        P.ctl[kRouteCtlLo] = P.doc_off[0];
        P.ctl[kRouteCtlHi] = P.doc_off[P.n_docs];
    }
}

__global__ void __launch_bounds__(kRouteBlock) k_route_place(const RouteParams P) {
    const WaveId w(kRouteBlock);
    const uint32_t lane = w.lane;
    for (uint64_t tile = w.wave; tile < P.n_tiles; tile += w.n_waves) {
        const uint64_t d = tile * kRouteTileDocs + lane;
        const bool in = d < P.n_docs;
        const uint64_t mem = in ? P.member[d] : 0ull;
        const uint32_t len = in ? P.len[d] : 0u;
        const uint64_t src = in ? P.doc_off[d] : 0ull;
        for (uint32_t b = 0; b < P.B; b++) {                        // (uniform, and so is the skip of a bucket the tile has nothing for)
            const uint64_t ballot = __ballot((mem >> b) & 1ull);
            if (!ballot) continue;
            if ((mem >> b) & 1ull) {
                const uint64_t r = route_rank(P.base[route_cell(b, P.n_tiles, tile)], ballot, lane);
                P.ent_len[r] = len;
                P.c_src[r] = src;
                if (r < P.cap_docs) P.doc_idx[r] = d;
            }
        }
    }
}

__global__ void __launch_bounds__(kRouteBlock) k_route_finish(const RouteParams P) {
    const uint64_t r = (uint64_t)blockIdx.x * kRouteBlock + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x <= P.B) P.ctl[kRouteCtlByte + threadIdx.x] = P.c_off[P.ctl[kRouteCtlDoc + threadIdx.x]];
    if (P.out_off && r <= P.m && r <= P.cap_docs) P.out_off[r] = P.c_off[r];
}

}  // namespace

hipError_t launch_route_mark(const RouteParams& P, unsigned n_cus, hipStream_t st) {
    if (!P.n_docs) return hipSuccess;
    const bool flat = P.W == 0 || P.n_buckets == 0;                 // (no words or no masks: a thread a document)
    k_route_mark<<<dim3(join_rows_grid(BitRows{P.bitmap, P.n_docs, P.W, P.lg, 0}, flat, n_cus)), dim3(kRouteBlock), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_route_count(const RouteParams& P, unsigned n_cus, hipStream_t st) {
    if (!P.n_tiles) return hipSuccess;
    k_route_count<<<dim3(wave_grid(P.n_tiles, kRouteBlock, n_cus)), dim3(kRouteBlock), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_route_pack(const RouteParams& P, hipStream_t st) {
    k_route_pack<<<dim3(1), dim3(kRouteBlock), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_route_place(const RouteParams& P, unsigned n_cus, hipStream_t st) {
    if (!P.n_tiles || !P.m) return hipSuccess;
    k_route_place<<<dim3(wave_grid(P.n_tiles, kRouteBlock, n_cus)), dim3(kRouteBlock), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_route_finish(const RouteParams& P, hipStream_t st) {
    // (one block at least: block 0 gathers the byte borders)
    const uint64_t n = P.out_off ? std::min(P.m, P.cap_docs) + 1 : 1;
    k_route_finish<<<dim3((unsigned)((n + kRouteBlock - 1) / kRouteBlock)), dim3(kRouteBlock), 0, st>>>(P);
    return hipGetLastError();
}

}  // namespace gft
