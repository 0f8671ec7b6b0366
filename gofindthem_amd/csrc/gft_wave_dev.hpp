// gft_wave_dev.hpp -- the lane kit of the wave64 kernels: values moved between the lanes of a wave, the wave's prefix sum,
// ballot rank and LDS fence, who a lane is in a grid of waves, and the grid such a kernel gets.  For .hip files, the scan
// kernels among them (their text loads and slots: gft_scan_dev.hpp).  (gft_kernels.hip keeps a prefix sum built from __shfl_up,
// wave_incl_scan_shfl: other code than the DPP form here.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

namespace gft {

__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }
// the value of the first active lane / of a lane that is the same in every lane: scalar values
__device__ __forceinline__ uint32_t first_lane32(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t first_lane64(uint64_t v) { return (uint64_t)first_lane32((uint32_t)(v >> 32)) << 32 | first_lane32((uint32_t)v); }
__device__ __forceinline__ uint32_t lane_value(uint32_t v, int lane) { return (uint32_t)__builtin_amdgcn_readlane((int)v, lane); }
__device__ __forceinline__ uint64_t lane_value64(uint64_t v, int lane) { return (uint64_t)lane_value((uint32_t)(v >> 32), lane) << 32 | lane_value((uint32_t)v, lane); }
// ... of a lane that is the same in every lane but computed in vector registers at run time: the lane number goes through
// readfirstlane (a scalar read instead of an LDS permute)
__device__ __forceinline__ uint32_t lane_value_at(uint32_t v, uint32_t l) {
    return __builtin_amdgcn_readlane(v, __builtin_amdgcn_readfirstlane(l));
}
// the value of a lane each lane names for itself, as two 32-bit halves
__device__ __forceinline__ uint64_t shuffle64(uint64_t v, int lane) {
    return (uint64_t)(uint32_t)__shfl((int)(v >> 32), lane, 64) << 32 | (uint32_t)__shfl((int)(uint32_t)v, lane, 64);
}
__device__ __forceinline__ uint64_t shuffle_xor64(uint64_t v, int s) {
    return (uint64_t)(uint32_t)__shfl_xor((int)(v >> 32), s, 64) << 32 | (uint32_t)__shfl_xor((int)(uint32_t)v, s, 64);
}
// the value of the lane s below / above (the lane's own where there is none): HIP's 64-bit overloads
__device__ __forceinline__ uint64_t up64(uint64_t v, uint32_t s) { return __shfl_up(v, s, 64); }
__device__ __forceinline__ uint64_t down64(uint64_t v, uint32_t s) { return __shfl_down(v, s, 64); }

// inclusive prefix sum over the 64 lanes with DPP moves (row shifts inside the four rows of 16 lanes, then the row
// totals are broadcast into the rows behind them): ten VALU instructions, no LDS traffic, no index arithmetic
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, true);    // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, true);    // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, true);    // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, true);    // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);   // row_bcast:15 -> rows 1 and 3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);   // row_bcast:31 -> rows 2 and 3
    return v;
}
// this lane's rank among the set bits of a ballot mask that lie below it: lanes with something to append take consecutive cells
__device__ __forceinline__ uint32_t wave_rank(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
}
// what the wave's lanes wrote to LDS before is seen by all of them behind: release, wave barrier, acquire
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// a lane's place in a one-dimensional grid of blocks of `block` threads (a multiple of 64)
struct WaveId {
    uint32_t lane;
    uint64_t wave, n_waves;
    __device__ __forceinline__ explicit WaveId(uint32_t block)
        : lane(threadIdx.x & 63u), wave(((uint64_t)blockIdx.x * block + threadIdx.x) >> 6), n_waves(((uint64_t)gridDim.x * block) >> 6) {}
};

// blocks of `block` threads for `waves` waves that have work: 8 blocks per CU at most, one at least
inline unsigned wave_grid(uint64_t waves, uint32_t block, unsigned n_cus) {
    const uint64_t blocks = std::min<uint64_t>((waves + block / 64 - 1) / (block / 64), (uint64_t)std::max(n_cus, 1u) * 8);
    return (unsigned)std::max<uint64_t>(blocks, 1);
}

}  // namespace gft
