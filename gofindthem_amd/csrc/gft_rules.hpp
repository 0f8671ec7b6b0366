// gft_rules.hpp -- rule evaluation for records on the device (gft_rules.hip): parameter block, launchers, and the engine's
// side of it (gft_rules_api.cpp) that group_records.cpp drives.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gft.h"
#include "rule_words.hpp"

namespace gft {

struct RuleSet;

struct RulesParams {
    const uint32_t* tag_rows;    // [n_leaves][TW] (k_leaf_tags)
    const uint32_t* leaf_field;  // [n_leaves]
    const uint64_t* rec_off;     // [n_records + 1]
    uint64_t n_records, n_leaves;
    const uint32_t* masks;       // [n_masks][FW]
    const uint32_t* units;       // [n_units][2] = tag id (kRuleNoTag: never), mask id
    const uint32_t* prog;        // postfix words of all rule expressions
    const uint32_t* prog_off;    // [n_rules + 1]
    uint32_t TW, FW, RW;         // words of a tag row, a field mask, a row of the result
    uint32_t n_fields, n_units, n_rules, max_depth;
    uint32_t* flags;             // [2]: a field index outside the schema; record offsets that descend or leave [0, n_leaves]
    uint32_t* out;               // [n_records][RW]
};

// what the flag words of a record batch say, read back after its kernels: GFT_OK, or GFT_E_INVALID and its message
int record_flags_rc(gft_engine* e, const uint32_t h_flags[2]);

size_t rules_lds_bytes(uint32_t n_units, uint32_t max_depth);
hipError_t launch_leaf_tags(const uint32_t* d_hit, uint32_t n_exprs, const uint32_t* d_expr_tag, const uint32_t* d_leaf_field, uint32_t n_fields,
                            uint64_t n_leaves, uint32_t n_tags, uint32_t* d_tag_rows, uint32_t* d_flags, hipStream_t st);
// hipErrorInvalidValue: the set's UNIT words and operand stacks do not fit lds_max
hipError_t launch_record_rules(const RulesParams& P, size_t lds_max, hipStream_t st);

}  // namespace gft

// ---- for group_records.cpp and group_json.cpp: the engine's side (gft_rules_api.cpp).  Single-device handles only (GFT_E_UNSUPPORTED otherwise); every
// call takes the engine's lock, which is recursive: a caller that needs several of them to see one state -- a group's call
// from set install to the read of the flags, next to another group on the same finder -- holds RulesLock around them.
namespace gft {

void rules_lock(gft_engine* e);
void rules_unlock(gft_engine* e);
struct RulesLock {
    gft_engine* e;
    explicit RulesLock(gft_engine* e_) : e(e_) { if (e) rules_lock(e); }
    ~RulesLock() { if (e) rules_unlock(e); }
    RulesLock(const RulesLock&) = delete;
    RulesLock& operator=(const RulesLock&) = delete;
};
// Uploads a compiled set; *serial names it (another group on the same finder may install its own: the caller compares).
int rules_install(gft_engine* e, const RuleSet& rs, uint64_t* serial);
uint64_t rules_serial(gft_engine* e);
// the engine-owned leaf bitmap of a record batch: n_leaves rows of `words` words, grown on demand (GFT_E_NOMEM)
int rules_leaf_bitmap(gft_engine* e, uint64_t n_leaves, uint32_t words, uint32_t** d_bitmap);
// host arrays -> engine-owned staging buffers (k < 6 of them, grown on demand), enqueued on the engine's stream and drained
int rules_stage(gft_engine* e, int n, const void* const* src, const uint64_t* bytes, const uint64_t* slack, void** d_dst);
int rules_fetch(gft_engine* e, void* dst, const void* d_src, uint64_t bytes);
// the two kernels over a leaf bitmap on the device; the rule bitmap is complete and the flags are read when this returns
// (GFT_E_INVALID: the batch named a field outside the schema, or its record offsets are broken -- checked also for a set
// without rules)
int rules_eval_device(gft_engine* e, const uint32_t* d_hit_bitmap, const uint32_t* d_leaf_field, const uint64_t* d_rec_off,
                      uint64_t n_records, uint64_t n_leaves, uint32_t* d_rule_bitmap);

}  // namespace gft
