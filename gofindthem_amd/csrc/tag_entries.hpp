// tag_entries.hpp -- the tag entries of a record batch on the host: the contract of gft_tags.hip stated in plain loops.  Pure: no
// device, no handle.  It is the fallback route of gft_group_tag_records, gft_debug_tag_entries, and what the device kernels are
// compared with.
#pragma once
#include <cstdint>

#include "rule_set.hpp"

namespace gft {

// hit rows [n_leaves][ceil(n_exprs / 32)] of a validated batch (validate_records) -> row_off [n_records + 1], always complete,
// and one entry per set bit e < n_exprs of every leaf whose field is valid (rs.valid): leaves in record order, e ascending
// inside a leaf; ent_tag (nullable) = rs.expr_tag[e].  An entry at a position >= cap is not stored; *total (nullable) =
// row_off[n_records].  A field named twice in a record contributes twice.
void tag_entries_host(const RuleSet& rs, const uint32_t* hit_bitmap, uint32_t n_exprs, const uint32_t* leaf_field, const uint64_t* rec_off,
                      uint64_t n_records, uint64_t n_leaves, uint64_t* row_off, uint32_t* ent_field, uint32_t* ent_expr, uint32_t* ent_tag,
                      uint64_t cap, uint64_t* total);

}  // namespace gft
