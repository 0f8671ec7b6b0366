// gft_json.hip -- a batch of raw JSON documents in HBM -> the record form of gft_group_process_records_device, gfx950 / wave64.
//
//   (blob, doc_off [n_docs + 1], schema trie)  ->  status [n_docs], rec_off [n_docs + 1], leaf_field, leaf_off, text
//
//   k_json<false>   status, leaves and decoded bytes per document                        -> status, cnt_leaves, cnt_text
//   (k_scan_* of gft_kernels.hip: cnt_leaves -> rec_off, cnt_text -> text_off)
//   k_json<true>    the same walk again over the documents of status 0: every leaf's field and offset, its bytes copied with a
//                   per-lane prefix count as the output position
//
//   k_json_paths    discovery, no trie: the distinct paths of the batch's string values into a set of path hashes and a pool
//                   (gft_group_json_paths_device; the host compiles them into the schema of gft_group_process_jsons_auto)
//
// A wave owns a document at a time and reads it in pieces of 64 bytes, a byte per lane; workgroups of four waves stride over
// the batch.  What a piece means is decided by gft_json_walk.hpp, which the host compiles too: here its lane operations are
// ballots, a shuffle reduction and v_readlane, its per-wave memory (visited bitset, container stack) is LDS.  The walk is
// latency bound -- one grammar step per structural byte, wave-uniform --, the copy of the leaves is coalesced.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gft_json.hpp"

namespace gft {

namespace {

constexpr uint32_t kJsonBlock = 256;        // 4 waves

struct DevWave {
    uint32_t lane, b, fl;
    JsonLaneOut lo;
    JsonWaveMem* m;
    __device__ void load(const uint8_t* doc, uint32_t base, uint32_t len) { b = (uint64_t)base + lane < len ? doc[base + lane] : 0u; }
    __device__ uint32_t lane_byte(uint32_t) const { return b; }
    __device__ uint32_t byte_at(uint32_t k) const { return (uint32_t)__builtin_amdgcn_readlane((int)b, (int)k); }
    template <class F> __device__ uint64_t ballot(F&& f) { return __ballot(f(lane) ? 1 : 0); }
    template <class F> __device__ uint32_t sum(F&& f) {
        uint32_t v = f(lane);
        for (int o = 32; o; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
        return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
    }
    template <class F> __device__ void each(F&& f) { f(lane); __builtin_amdgcn_wave_barrier(); }
    template <class F> __device__ void once(F&& f) { if (lane == 0) f(); }
    __device__ JsonLaneOut& out(uint32_t) { return lo; }
    __device__ uint32_t& flags(uint32_t) { return fl; }
    __device__ uint32_t uni(uint32_t x) const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
    __device__ JsonWaveMem& mem() { return *m; }
};

template <bool WRITE>
__global__ void __launch_bounds__(kJsonBlock) k_json(const JsonParams P) {
    __shared__ JsonWaveMem s_mem[kJsonBlock / 64];
    DevWave w;
    w.lane = threadIdx.x & 63u;
    w.m = &s_mem[threadIdx.x >> 6];
    const uint64_t wave = ((uint64_t)blockIdx.x * kJsonBlock + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * kJsonBlock) >> 6;
    if (WRITE && P.leaf_off && blockIdx.x == 0 && threadIdx.x == 0 && P.rec_off[P.n_docs] <= P.leaf_cap)
        P.leaf_off[P.rec_off[P.n_docs]] = P.text_off[P.n_docs];
    for (uint64_t d = wave; d < P.n_docs; d += n_waves) {
        const uint64_t a = P.doc_off[d], z = P.doc_off[d + 1];
        uint32_t n_leaves = 0, n_text = 0;
        if (!WRITE) {
            uint32_t st = kJsSyntax;
            if (z < a || z - a > 0xFFFFFFFFull) {
                if (w.lane == 0) atomicOr(P.flags, 1u);
            } else {
                const JsonDocOut none{nullptr, nullptr, nullptr, 0, 0, 0, 0};
                st = json_walk_doc(w, P.T, P.blob + a, (uint32_t)(z - a), none, &n_leaves, &n_text);
            }
            if (w.lane == 0) { P.status[d] = (uint8_t)st; P.cnt_leaves[d] = n_leaves; P.cnt_text[d] = n_text; }
        } else {
            if (P.status[d] || !P.cnt_leaves[d]) continue;
            const bool leaves = P.leaf_cap && P.leaf_off;
            const JsonDocOut O{leaves ? P.leaf_field : nullptr, leaves ? P.leaf_off : nullptr, P.text_cap ? P.text : nullptr,
                               P.leaf_cap, P.text_cap, P.rec_off[d], P.text_off[d]};
            (void)json_walk_doc(w, P.T, P.blob + a, (uint32_t)(z - a), O, &n_leaves, &n_text);
        }
    }
}

// the wave of k_json_paths: what discovery needs on top (gft_json_walk.hpp).  One lane issues an atomic, every lane gets
// its answer; the set's slot is read by a load of device scope, which sees what another wave's compare-and-swap put there.
struct DevPathWave : DevWave {
    __device__ uint64_t uni64(uint64_t x) const { return (uint64_t)uni((uint32_t)(x >> 32)) << 32 | uni((uint32_t)x); }
    template <class F> __device__ uint64_t sum64(F&& f) {
        const uint64_t v = f(lane);
        uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
        for (int o = 32; o; o >>= 1) {                                       // (64-bit adds: the carry goes with the halves)
            const uint64_t other = (uint64_t)(uint32_t)__shfl_xor((int)hi, o, 64) << 32 | (uint32_t)__shfl_xor((int)lo, o, 64);
            const uint64_t s = ((uint64_t)hi << 32 | lo) + other;
            lo = (uint32_t)s; hi = (uint32_t)(s >> 32);
        }
        return uni64((uint64_t)hi << 32 | lo);
    }
    __device__ uint64_t load64(const uint64_t* p) const { return uni64(__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)); }
    __device__ uint64_t cas64(uint64_t* p, uint64_t v) const {
        unsigned long long old = 0;
        if (lane == 0) old = atomicCAS(reinterpret_cast<unsigned long long*>(p), 0ull, (unsigned long long)v);
        return uni64(old);
    }
    __device__ uint32_t add32(uint32_t* p, uint32_t v) const {
        uint32_t old = 0;
        if (lane == 0) old = atomicAdd(p, v);
        return uni(old);
    }
};

__global__ void __launch_bounds__(kJsonBlock) k_json_paths(const JsonPathParams P) {
    __shared__ JsonWaveMem s_mem[kJsonBlock / 64];
    __shared__ JsonPathMem s_pm[kJsonBlock / 64];
    DevPathWave w;
    w.lane = threadIdx.x & 63u;
    w.m = &s_mem[threadIdx.x >> 6];
    JsonPaths dsc{&s_pm[threadIdx.x >> 6], P.set};
    const uint64_t wave = ((uint64_t)blockIdx.x * kJsonBlock + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * kJsonBlock) >> 6;
    for (uint64_t d = wave; d < P.n_docs; d += n_waves) {
        const uint64_t a = P.doc_off[d], z = P.doc_off[d + 1];
        if (z < a || z - a > 0xFFFFFFFFull) {
            if (w.lane == 0) atomicOr(P.flags, 1u);
            continue;
        }
        json_walk_paths(w, dsc, P.blob + a, (uint32_t)(z - a));
    }
}

unsigned json_grid(uint64_t n_docs, unsigned n_cus) {
    const uint64_t blocks = (n_docs + kJsonBlock / 64 - 1) / (kJsonBlock / 64);
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(blocks, (uint64_t)std::max(n_cus, 1u) * 8));   // 32 waves per CU
}

}  // namespace

hipError_t launch_json_count(const JsonParams& P, unsigned n_cus, hipStream_t st) {
    if (!P.n_docs) return hipSuccess;
    k_json<false><<<dim3(json_grid(P.n_docs, n_cus)), dim3(kJsonBlock), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_json_write(const JsonParams& P, unsigned n_cus, hipStream_t st) {
    if (!P.n_docs) return hipSuccess;
    k_json<true><<<dim3(json_grid(P.n_docs, n_cus)), dim3(kJsonBlock), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_json_paths(const JsonPathParams& P, unsigned n_cus, hipStream_t st) {
    if (!P.n_docs) return hipSuccess;
    k_json_paths<<<dim3(json_grid(P.n_docs, n_cus)), dim3(kJsonBlock), 0, st>>>(P);
    return hipGetLastError();
}

}  // namespace gft
