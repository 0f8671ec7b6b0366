// tag_entries.cpp -- tag_entries_host (tag_entries.hpp): a bit at a time, a leaf at a time, a record at a time.
#include "tag_entries.hpp"

namespace gft {

void tag_entries_host(const RuleSet& rs, const uint32_t* hit_bitmap, uint32_t n_exprs, const uint32_t* leaf_field, const uint64_t* rec_off,
                      uint64_t n_records, uint64_t n_leaves, uint64_t* row_off, uint32_t* ent_field, uint32_t* ent_expr, uint32_t* ent_tag,
                      uint64_t cap, uint64_t* total) {
    const uint64_t EW = (n_exprs + 31) / 32;
    uint64_t at = 0;
    for (uint64_t r = 0; r < n_records; r++) {
        row_off[r] = at;
        for (uint64_t l = rec_off[r]; l < rec_off[r + 1] && l < n_leaves; l++) {
            const uint32_t f = leaf_field[l];
            if (f >= rs.n_fields || !(rs.valid[f >> 5] >> (f & 31) & 1u)) continue;
            const uint32_t* row = hit_bitmap + l * EW;
            for (uint32_t e = 0; e < n_exprs; e++) {
                if (!row[e >> 5]) { e |= 31; continue; }             // (an empty word: on to the next)
                if (!(row[e >> 5] >> (e & 31) & 1u)) continue;
                if (at < cap) {
                    ent_field[at] = f;
                    ent_expr[at] = e;
                    if (ent_tag) ent_tag[at] = rs.expr_tag[e];
                }
                at++;
            }
        }
    }
    row_off[n_records] = at;
    if (total) *total = at;
}

}  // namespace gft
