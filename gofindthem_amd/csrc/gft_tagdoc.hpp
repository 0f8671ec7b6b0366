// gft_tagdoc.hpp -- the tag result document of a record batch written on the device (gft_tagdoc.hip): parameter block,
// launchers, and the engine's side of it (gft_tagdoc_api.cpp) that group_json.cpp and group_tags.cpp drive.  The text format,
// the tables and the pure host statement of the same contract are tags_json.hpp's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gft.h"

namespace gft {

struct TagSlots;
struct TagFields;

// flag words of a call (plain stores of 1)
enum : uint32_t {
    kTagDocFlagField = 0,    // a leaf names a field outside the schema
    kTagDocFlagOffsets,      // record offsets that descend, leave [0, n_leaves] or do not end at n_leaves
    kTagDocFlagHole,         // a hole of 4 GiB or more
    kTagDocFlagTwice,        // a record names a valid field twice
    kTagDocFlagLeaves,       // a record of more than GFT_TAGS_JSON_MAX_LEAVES leaves that is not a hole
    kTagDocFlagLong,         // a document whose length + 1 does not fit 32 bits
    kTagDocFlags = 8
};

struct TagDocParams {
    const uint32_t* hits;        // [n_leaves][EW] leaf hit rows (k_tag_slots only)
    uint32_t EW;
    uint32_t* slot_rows;         // [n_leaves][SW]: written by k_tag_slots, read by k_tagdoc
    const uint32_t* leaf_field;  // [n_leaves]
    const uint64_t* rec_off;     // [n_records + 1]
    uint64_t n_leaves, n_records;
    const uint64_t* hole_len;    // [n_records], nullable: != 0 reserves that many bytes and the record's leaves are not read
    // the slot table (TagSlots) and its blob
    uint32_t SW, n_tags;
    const uint32_t* src_off; const uint32_t* src_expr; const uint32_t* slot_off; const uint32_t* slot_len;
    const uint32_t* tag_word; const uint32_t* tag_words; const uint32_t* tag_off; const uint32_t* tag_len;
    const uint8_t* slot_blob;
    // the field table (TagFields) and its blob
    uint32_t n_fields;
    const uint32_t* field_rank; const uint32_t* field_off; const uint32_t* field_len; const uint32_t* valid;
    const uint8_t* field_blob;
    uint32_t* flags;             // [kTagDocFlags]
    uint32_t* cnt;               // count pass: [n_records] len(d) + 1
    // fill pass
    const uint64_t* scan;        // [n_records + 1] exclusive scan of cnt
    uint64_t* out_off;           // [n_records + 1] = 1 + scan
    uint8_t* out;                // [cap]
    uint64_t cap;
};

// slot_rows[l][w]: bit s of a word is the OR of the hit bits of slot s's expressions; zero for a leaf whose field is invalid or
// outside the schema (kTagDocFlagField), whose hit row is not read
hipError_t launch_tag_slots(const TagDocParams& P, hipStream_t st);
// cnt[d] = len(d) + 1: the document (or its hole) and the separator behind it; the record offsets are checked here
hipError_t launch_tagdoc_count(const TagDocParams& P, unsigned n_cus, hipStream_t st);
// out_off, the frame and the fragments; nothing at or past cap, nothing of a hole.  n_records == 0: "[]" and out_off[0] = 1
hipError_t launch_tagdoc_fill(const TagDocParams& P, unsigned n_cus, hipStream_t st);

// ---- the engine's side (gft_tagdoc_api.cpp).  Single-device handles only (GFT_E_UNSUPPORTED otherwise); the calls take the
// engine's (recursive) lock.  The tables and the scratch -- slot rows, counts, scan, partials, flags, the staged leaf fields and
// record offsets, the owned text -- are the engine's own (d_tagdoc), apart from every other call's.
// Uploads the tables that are given (either may be null); *serial names the copy (another group on the same finder installs its
// own: the caller compares)
int tags_json_install(gft_engine* e, const TagSlots* slots, uint64_t* slot_serial, const TagFields* fields, uint64_t* field_serial);
void tags_json_serials(gft_engine* e, uint64_t* slot_serial, uint64_t* field_serial);
// Every pointer is a device pointer except total.  Complete when it returns.  Cap protocol of gft_compact_device: d_out_off
// always complete, nothing stored at or past cap, *total = the text's size, GFT_OK either way; d_out == NULL with cap == 0
// counts only.  GFT_E_INVALID: no tables installed, a hole of 4 GiB or more, what rules_eval_device refuses of a batch.
// GFT_E_UNSUPPORTED: what tags_json_host refuses (the text of the failure names it); the handle answers afterwards.
int tags_json_device(gft_engine* e, const uint32_t* d_hit_bitmap, const uint32_t* d_leaf_field, const uint64_t* d_rec_off, uint64_t n_records,
                     uint64_t n_leaves, const uint64_t* d_hole_len, uint8_t* d_out, uint64_t cap, uint64_t* d_out_off, uint64_t* total);
// The same in two steps, for a caller whose leaf bitmap does not outlive its next finder call: the slot rows, and copies of the
// leaf fields and the record offsets, into the engine's own buffers (*d_rec_off_kept names the copy of the offsets) ...
int tags_json_stage(gft_engine* e, const uint32_t* d_hit_bitmap, const uint32_t* d_leaf_field, const uint64_t* d_rec_off, uint64_t n_records,
                    uint64_t n_leaves, const uint64_t** d_rec_off_kept);
// ... and the text of the staged batch into a buffer the engine owns: counted first, grown to the total (GFT_E_NOMEM), then
// filled.  h_hole_len: host memory, nullable, uploaded into the engine's own buffer.
int tags_json_owned(gft_engine* e, const uint64_t* h_hole_len, const uint8_t** d_text, const uint64_t** d_out_off, uint64_t* total);

}  // namespace gft
