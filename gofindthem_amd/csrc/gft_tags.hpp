// gft_tags.hpp -- tag entries on the device (gft_tags.hip): a record batch's leaf hit bitmap -> per-record sparse lists of
// (field, expression), the batch form of TagObject's map.  Parameter block, launchers, and the engine's side of it
// (gft_tags_api.cpp) that group_tags.cpp drives.  The pure host statement of the same contract is tag_entries_host
// (tag_entries.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gft.h"
#include "gft_bitrows_dev.hpp"

namespace gft {

struct TagParams {
    BitRows rows;                // [n_leaves][W] hit rows: a row a leaf (bit_rows)
    const uint32_t* leaf_field;  // [n_leaves]
    const uint32_t* valid;       // [ceil(n_fields / 32)] RuleSet::valid
    uint32_t n_fields;
    uint32_t* flags;             // [2]: a field index outside the schema; record offsets that descend or leave [0, n_leaves]
    uint32_t* cnt;               // count pass: [n_leaves]
    // fill pass
    const uint64_t* leaf_ent_off;  // [n_leaves + 1] exclusive scan of cnt
    const uint64_t* rec_off;       // [n_records + 1]
    uint64_t n_records;
    uint64_t* row_off;             // [n_records + 1]
    uint32_t* ent_field;           // [cap]
    uint32_t* ent_expr;            // [cap]
    uint32_t* ent_tag;             // [cap], nullable
    const uint32_t* expr_tag;      // [n_exprs]
    uint64_t cap;
};

// cnt[l] = set bits < n_exprs of leaf l's row, 0 when its field is invalid or outside the schema (flags[0])
hipError_t launch_tags_count(const TagParams& P, unsigned n_cus, hipStream_t st);
// row_off[r] = leaf_ent_off[rec_off[r]] for r = 0 .. n_records (offsets checked first: flags[1]), then the entries below cap
hipError_t launch_tags_fill(const TagParams& P, unsigned n_cus, hipStream_t st);

// ---- the engine's side (gft_tags_api.cpp).  Single-device handles only; the calls take the engine's (recursive) lock, the set
// must have been installed (rules_install).  Scratch -- counts, leaf offsets, scan partials -- is the engine's own, apart from
// the compaction's and the rule kernels'.
// Every pointer is a device pointer except total.  Complete when it returns: the three launches ran and the flags were read
// (GFT_E_INVALID as rules_eval_device).  Cap protocol of gft_compact_device: row_off always complete, nothing stored at or
// past cap, *total = row_off[n_records], GFT_OK either way; NULL arrays with cap == 0 count only.
int rules_tag_entries_device(gft_engine* e, const uint32_t* d_hit_bitmap, const uint32_t* d_leaf_field, const uint64_t* d_rec_off,
                             uint64_t n_records, uint64_t n_leaves, uint64_t* d_row_off, uint32_t* d_ent_field, uint32_t* d_ent_expr,
                             uint32_t* d_ent_tag, uint64_t cap, uint64_t* total);
// ... into arrays the engine owns: counted first, grown to the total, then filled (one count pass, one fill pass)
int rules_tag_entries_owned(gft_engine* e, const uint32_t* d_hit_bitmap, const uint32_t* d_leaf_field, const uint64_t* d_rec_off,
                            uint64_t n_records, uint64_t n_leaves, const uint64_t** d_row_off, const uint32_t** d_ent_field,
                            const uint32_t** d_ent_expr, uint64_t* total);

}  // namespace gft
