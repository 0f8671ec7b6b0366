// gft_result.hpp -- the result document of a batch's rule rows written on the device (gft_result.hip): parameter block,
// launchers, and the engine's side of it (gft_result_api.cpp) that group_json.cpp drives.  The text format, the fragment
// table and the pure host statement of the same contract are rules_json.hpp's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gft.h"

namespace gft {

struct RuleFragments;

struct ResultParams {
    const uint32_t* rows;        // [n_docs][RW] rule rows
    uint64_t n_docs;
    uint32_t R, RW;              // rule expressions (bits of a row), words of a row
    const uint64_t* hole_len;    // [n_docs], nullable: != 0 reserves that many bytes and the row is not read
    // the fragment table (RuleFragments), [R] each, and its blob with 16 readable bytes behind it
    const uint32_t* rule_first; const uint32_t* name_off; const uint32_t* name_len; const uint32_t* expr_off; const uint32_t* expr_len;
    const uint8_t* blob;
    uint32_t* flags;             // [2]: a hole of 4 GiB or more
    uint32_t* cnt;               // count pass: [n_docs] len(d) + 1
    // fill pass
    const uint64_t* scan;        // [n_docs + 1] exclusive scan of cnt
    uint64_t* out_off;           // [n_docs + 1] = 1 + scan
    uint8_t* out;                // [cap]
    uint64_t cap;
};

// cnt[d] = len(d) + 1: the document (or its hole) and the separator behind it
hipError_t launch_result_count(const ResultParams& P, unsigned n_cus, hipStream_t st);
// out_off, the frame and the fragments; nothing at or past cap, nothing of a hole.  n_docs == 0: "[]" and out_off[0] = 1
hipError_t launch_result_fill(const ResultParams& P, unsigned n_cus, hipStream_t st);

// ---- the engine's side (gft_result_api.cpp).  Single-device handles only (GFT_E_UNSUPPORTED otherwise); the calls take the
// engine's (recursive) lock.  The table and the scratch -- counts, scan, partials, flags, the owned text -- are the engine's
// own (d_result), apart from the compaction's, the rule kernels' and the tag entries'.
// Uploads a fragment table; *serial names it (another group on the same finder installs its own: the caller compares)
int rules_json_install(gft_engine* e, const RuleFragments& fr, uint64_t* serial);
uint64_t rules_json_serial(gft_engine* e);
// Every pointer is a device pointer except total.  Complete when it returns.  Cap protocol of gft_compact_device: d_out_off
// always complete, nothing stored at or past cap, *total = the text's size, GFT_OK either way; d_out == NULL with cap == 0
// counts only.  GFT_E_INVALID: no table installed, a hole of 4 GiB or more.
int rules_json_device(gft_engine* e, const uint32_t* d_rule_bitmap, uint64_t n_docs, const uint64_t* d_hole_len, uint8_t* d_out, uint64_t cap,
                      uint64_t* d_out_off, uint64_t* total);
// ... into a text buffer the engine owns: counted first, grown to the total (GFT_E_NOMEM), then filled.  h_hole_len: host
// memory, nullable, uploaded into the engine's own buffer.
int rules_json_owned(gft_engine* e, const uint32_t* d_rule_bitmap, uint64_t n_docs, const uint64_t* h_hole_len, const uint8_t** d_text,
                     const uint64_t** d_out_off, uint64_t* total);

}  // namespace gft
