// gft_stats_dev.hpp -- "is this entry the first of its (document, term) pair" on the device, for the kernels that walk a term list
// by the steps of gft_stats_piece.hpp: the term statistics' docs counter (gft_stats.hip) and the distinct scores (gft_rank.hip).
// The step's set and the large path's bitset are the caller's memory; who empties them and when is in the kernels.
#pragma once
#include <hip/hip_runtime.h>

#include "gft_stats_piece.hpp"

namespace gft {

// a step's relative offsets in LDS, as stats_step_docs / stats_find_doc read them
struct LdsRel {
    const uint32_t* p;
    __device__ __forceinline__ uint32_t operator[](uint32_t k) const { return p[k]; }
};

// (document dl of the step, term t) into the step's set [kStatsSetSlots]: true for the lane that entered the pair, with the slot it
// took in `mine` -- the lane zeroes that slot once every lane of the workgroup has asked
__device__ __forceinline__ bool stats_set_first(uint64_t* s_set, uint32_t dl, uint32_t t, uint32_t& mine) {
    const uint64_t key = stats_set_key(dl, t);
    for (uint32_t s = stats_set_slot(dl, t);; s = stats_set_next(s)) {
        const uint64_t old = atomicCAS(reinterpret_cast<unsigned long long*>(&s_set[s]), 0ull, (unsigned long long)key);
        if (old == 0) { mine = s; return true; }
        if (old == key) return false;
    }
}

// term t into a large document's bitset (LDS, or the workgroup's global row): true for the lane that set the bit
__device__ __forceinline__ bool stats_bitset_first(uint32_t* bits, uint32_t t) {
    const uint32_t bit = 1u << (t & 31u);
    return !(atomicOr(&bits[t >> 5], bit) & bit);
}

}  // namespace gft
