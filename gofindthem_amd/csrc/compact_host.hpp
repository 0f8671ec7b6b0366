// compact_host.hpp -- the host restatement of gft_compact.hip: hit bitmap -> per-document lists of true expressions.
#pragma once
#include <cstdint>

namespace gft {

// bitmap [n_docs][ceil(n_exprs / 32)] -> row_off [n_docs + 1] (always complete), expr_idx / label [min(total, cap)]
// (ascending inside a document; label nullable, label[k] = labels[expr_idx[k]]).  Bits at and above n_exprs are ignored;
// nothing is stored at or past `cap` entries.  Returns the total.
uint64_t compact_host(const uint32_t* bitmap, uint64_t n_docs, uint32_t n_exprs, const uint32_t* labels, uint64_t* row_off,
                      uint32_t* expr_idx, uint32_t* label, uint64_t cap);

}  // namespace gft
