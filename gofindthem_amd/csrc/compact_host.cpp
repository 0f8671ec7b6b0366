// compact_host.cpp -- hit bitmap -> CSR of the true expressions on the host: what gft_compact.hip does on the device, for
// bitmaps that were completed on the host (regex pass, host-solved expressions, several devices) and for the tests.
#include "compact_host.hpp"

#include <string>

#include "../../include/gft.h"
#include "gft_guard.hpp"

namespace gft {

uint64_t compact_host(const uint32_t* bitmap, uint64_t n_docs, uint32_t n_exprs, const uint32_t* labels, uint64_t* row_off,
                      uint32_t* expr_idx, uint32_t* label, uint64_t cap) {
    const uint64_t words = ((uint64_t)n_exprs + 31) / 32;
    const uint32_t tail = (n_exprs & 31) ? (1u << (n_exprs & 31)) - 1 : 0xFFFFFFFFu;
    uint64_t pos = 0;
    for (uint64_t d = 0; d < n_docs; d++) {
        row_off[d] = pos;
        const uint32_t* row = bitmap + d * words;
        for (uint64_t j = 0; j < words; j++) {
            uint32_t w = row[j] & (j + 1 == words ? tail : 0xFFFFFFFFu);
            while (w) {
                const uint32_t x = (uint32_t)j * 32u + (uint32_t)__builtin_ctz(w);
                w &= w - 1;
                if (pos < cap) {
                    if (expr_idx) expr_idx[pos] = x;
                    if (label) label[pos] = labels[x];
                }
                pos++;
            }
        }
    }
    row_off[n_docs] = pos;
    return pos;
}

}  // namespace gft

extern "C" int gft_debug_compact_host(const uint32_t* bitmap, uint64_t n_docs, uint32_t n_exprs, const uint32_t* labels,
                                      uint64_t* row_off, uint32_t* expr_idx, uint32_t* label, uint64_t cap, uint64_t* total) try {
    if (!row_off || (n_docs && n_exprs && !bitmap) || (cap && !expr_idx) || (label && !labels)) return GFT_E_INVALID;
    const uint64_t t = gft::compact_host(bitmap, n_docs, n_exprs, labels, row_off, expr_idx, label, cap);
    if (total) *total = t;
    return GFT_OK;
} GFT_CATCH(nullptr)
