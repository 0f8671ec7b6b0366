// gft_bitrows.hpp -- a hit bitmap's rows as the kernels that walk them take them (gft_bitrows_dev.hpp, gft_select.hip, gft_route.hip)
#pragma once
#include <stdint.h>

namespace gft {

// a row of W <= 64 words is a segment of 1 << lg lanes: W rounded up to a power of two (6 above that, where it is not read)
inline uint32_t bit_row_lg(uint32_t W) {
    uint32_t lg = 0;
    while ((1u << lg) < W && lg < 6) lg++;
    return lg;
}

}  // namespace gft
