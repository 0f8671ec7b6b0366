// gft_split.hpp -- a resident blob cut into line documents (gft_split.hip): the launchers, and the same walk on the host
// (split_host.cpp), which is also what a group finder without the device route splits with.
#pragma once
#include <stdint.h>

#include "../../include/gft.h"
#include "gft_split_piece.hpp"

namespace gft {

// gft_split_lines_device's contract on host pointers, tile by tile through gft_split_piece.hpp with the kernels' carry
// resolution; reads blob[0, len) only.  Returns a gft_status.
int split_lines_host(const uint8_t* blob, uint64_t len, uint32_t mode, uint64_t* doc_off, uint64_t cap, uint64_t* n_docs);

inline uint64_t split_tiles(uint64_t len) { return (len + kSplitTile - 1) / kSplitTile; }

}  // namespace gft

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace gft {

struct SplitParams {
    const uint8_t* blob;
    uint64_t len, n_tiles;
    SplitSum* sums;            // [n_tiles]      GFT_SPLIT_JSON_LINES: count pass -> carry pass
    SplitCarry* carry;         // [n_tiles]      carry pass -> write pass
    uint32_t* cnt;             // [n_tiles]      documents that start in the tile (the newline, or the first byte, lies in it)
    const uint64_t* base;      // [n_tiles + 1]  their exclusive prefix sum
    uint64_t* out;
    uint64_t cap;
};

hipError_t launch_split_count(const SplitParams& P, uint32_t mode, hipStream_t st);
hipError_t launch_split_carry(const SplitParams& P, hipStream_t st);
hipError_t launch_split_write(const SplitParams& P, uint32_t mode, hipStream_t st);

}  // namespace gft
#endif
