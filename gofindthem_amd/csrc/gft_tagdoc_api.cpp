// gft_tagdoc_api.cpp -- the tag result document of a record batch (gft_tagdoc.hpp): the engine's side, which group_json.cpp,
// group_tags.cpp and gft_group_tags_json_device drive.
#include "gft_engine.hpp"

#include <atomic>

#include "gft_tagdoc.hpp"
#include "tags_json.hpp"

using namespace gft;
using namespace gft::api;

namespace {

constexpr RoomTexts kTagDocRoom{"no device memory for the tag document's work buffers", "tag document alloc"};

int tagdoc_entry_checks(gft_engine* e) {
    if (!e->peers.empty()) return fail(e, GFT_E_UNSUPPORTED, "tag document: single-device handles only");
    return check_ready(e, kNeedDevice | kNeedSettled, "tag document");
}

int tagdoc_flags_rc(gft_engine* e, const uint32_t* h) {
    if (h[kTagDocFlagOffsets]) return fail(e, GFT_E_INVALID, "record batch: rec_off descends or does not end at n_leaves");
    if (h[kTagDocFlagField]) return fail(e, GFT_E_INVALID, "record batch: a leaf names a field outside the schema");
    if (h[kTagDocFlagHole]) return fail(e, GFT_E_INVALID, std::string("tag document: ") + tags_json_refusal_text(kTagsJsonHole));
    const int refusal = h[kTagDocFlagTwice] ? kTagsJsonTwice : h[kTagDocFlagLeaves] ? kTagsJsonLeaves : h[kTagDocFlagLong] ? kTagsJsonLong : kTagsJsonOk;
    if (refusal) return fail(e, GFT_E_UNSUPPORTED, std::string("tag document: ") + tags_json_refusal_text(refusal));
    return GFT_OK;
}

// the tables' part of the parameter block
void table_params(const gft_engine::TagDocBufs& T, TagDocParams& P) {
    P.SW = T.SW; P.n_tags = T.n_tags; P.n_fields = T.n_fields; P.EW = (T.n_exprs + 31) / 32;
    P.src_off = T.src_off.as<uint32_t>(); P.src_expr = T.src_expr.as<uint32_t>();
    P.slot_off = T.slot_off.as<uint32_t>(); P.slot_len = T.slot_len.as<uint32_t>();
    P.tag_word = T.tag_word.as<uint32_t>(); P.tag_words = T.tag_words.as<uint32_t>();
    P.tag_off = T.tag_off.as<uint32_t>(); P.tag_len = T.tag_len.as<uint32_t>(); P.slot_blob = T.slot_blob.as<uint8_t>();
    P.field_rank = T.field_rank.as<uint32_t>(); P.field_off = T.field_off.as<uint32_t>(); P.field_len = T.field_len.as<uint32_t>();
    P.valid = T.valid.as<uint32_t>(); P.field_blob = T.field_blob.as<uint8_t>();
    P.flags = T.flags.as<uint32_t>();
}

int batch_checks(gft_engine* e, const uint32_t* d_hit_bitmap, const uint32_t* d_leaf_field, const uint64_t* d_rec_off, uint64_t n_records,
                 uint64_t n_leaves) {
    int rc = tagdoc_entry_checks(e);
    if (rc) return rc;
    const auto& T = e->d_tagdoc;
    if (!T.slot_serial || !T.field_serial) return fail(e, GFT_E_INVALID, "tag document: no tables installed");
    if (!n_records && n_leaves) return fail(e, GFT_E_INVALID, "record batch: leaves but no records");
    if ((n_records && !d_rec_off) || (n_leaves && (!d_leaf_field || (T.n_exprs && !d_hit_bitmap))))
        return fail(e, GFT_E_INVALID, "record batch: null argument");
    return GFT_OK;
}

// the flags cleared, then the slot rows of the batch into the engine's own buffer
int slot_rows(gft_engine* e, TagDocParams& P, const uint32_t* d_hit_bitmap, const uint32_t* d_leaf_field, uint64_t n_leaves) {
    auto& T = e->d_tagdoc;
    int rc;
    if ((rc = room(e, T.flags, kTagDocFlags * 4, kTagDocRoom)) || (rc = room(e, T.slot_rows, n_leaves * T.SW * 4, kTagDocRoom))) return rc;
    table_params(T, P);
    P.hits = d_hit_bitmap; P.leaf_field = d_leaf_field; P.n_leaves = n_leaves; P.slot_rows = T.slot_rows.as<uint32_t>();
    HIP_TRY(hipMemsetAsync(P.flags, 0, kTagDocFlags * 4, e->stream), "tag document");
    ProfScope ps(e, "tagdoc_slots");
    HIP_TRY(launch_tag_slots(P, e->stream), "tag slot kernel launch");
    return GFT_OK;
}

// count, scan, the total and the flags, (owned: room for the total,) fill.  P: the tables, the slot rows and the batch.
// d_out_off == nullptr: the engine's own arrays, returned in d_out / d_out_off.
int tagdoc_text(gft_engine* e, TagDocParams& P, uint8_t*& d_out, uint64_t cap, uint64_t*& d_out_off, bool owned, uint64_t* total) {
    auto& T = e->d_tagdoc;
    hipStream_t st = e->stream;
    const uint64_t n = P.n_records;
    int rc;
    if (owned) {
        if ((rc = room(e, T.out_off, (n + 1) * 8, kTagDocRoom))) return rc;
        d_out_off = T.out_off.as<uint64_t>();
    }
    if (!d_out_off) return fail(e, GFT_E_INVALID, "tag document: null argument");
    if (!owned && cap && !d_out) return fail(e, GFT_E_INVALID, "tag document: a cap but no text buffer");
    if ((rc = room(e, T.cnt, n * 4, kTagDocRoom)) || (rc = room(e, T.scan, (n + 1) * 8, kTagDocRoom)) ||
        (rc = room(e, T.partial, scan_partials_needed(n) * 8, kTagDocRoom)))
        return rc;
    P.cnt = T.cnt.as<uint32_t>();
    uint64_t h_total = 1;                  // (n_records == 0: "[]", with the closing bracket added below)
    if (n) {
        {
            ProfScope ps(e, "tagdoc_count");
            HIP_TRY(launch_tagdoc_count(P, e->n_cus, st), "tag document count kernel launch");
        }
        {
            ProfScope ps(e, "tagdoc_scan");
            HIP_TRY(launch_exclusive_scan(P.cnt, n, T.scan.as<uint64_t>(), T.partial.as<uint64_t>(), st), "tag document scan");
        }
        // the one read between the passes: the total sizes the owned text, and a refused batch stops the call before the fill
        uint32_t h_flags[kTagDocFlags] = {};
        HIP_TRY(hipMemcpyAsync(h_flags, P.flags, sizeof h_flags, hipMemcpyDeviceToHost, st), "tag document");
        HIP_TRY(hipMemcpyAsync(&h_total, T.scan.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, st), "tag document");
        HIP_TRY(hipStreamSynchronize(st), "tag document");
        if ((rc = tagdoc_flags_rc(e, h_flags))) return rc;
    }
    h_total += 1;                          // the opening bracket
    if (owned) {
        if ((rc = room(e, T.text, h_total, kTagDocRoom))) return rc;
        d_out = T.text.as<uint8_t>();
        cap = h_total;
    }
    P.scan = T.scan.as<uint64_t>(); P.out_off = d_out_off; P.out = d_out; P.cap = d_out ? cap : 0;
    {
        ProfScope ps(e, "tagdoc_fill");
        HIP_TRY(launch_tagdoc_fill(P, e->n_cus, st), "tag document fill kernel launch");
    }
    HIP_TRY(hipStreamSynchronize(st), "tag document");
    if (total) *total = h_total;
    return GFT_OK;
}

}  // namespace

namespace gft {

int tags_json_install(gft_engine* e, const TagSlots* slots, uint64_t* slot_serial, const TagFields* fields, uint64_t* field_serial) try {
    if (!e || (slots && !slot_serial) || (fields && !field_serial)) return GFT_E_INVALID;
    GFT_LOCK(e);
    int rc = tagdoc_entry_checks(e);
    if (rc) return rc;
    DeviceGuard g(e->device);
    auto& T = e->d_tagdoc;
    static std::atomic<uint64_t> next_serial{1};
    const char* what = "tag document table upload";
    T.staged = false;                      // (slot rows of another table are no batch of this one)
    if (slots) {
        const TagSlots& s = *slots;
        T.slot_serial = 0;                 // (a failed upload leaves no table)
        if ((rc = upload(e, T.src_off, s.src_off, what)) || (rc = upload(e, T.src_expr, s.src_expr, what)) ||
            (rc = upload(e, T.slot_off, s.slot_off, what)) || (rc = upload(e, T.slot_len, s.slot_len, what)) ||
            (rc = upload(e, T.tag_word, s.tag_word, what)) || (rc = upload(e, T.tag_words, s.tag_words, what)) ||
            (rc = upload(e, T.tag_off, s.tag_off, what)) || (rc = upload(e, T.tag_len, s.tag_len, what)) ||
            (rc = upload(e, T.slot_blob, s.blob, what)))
            return rc;
        HIP_TRY(hipStreamSynchronize(e->stream), what);
        T.n_exprs = s.n_exprs; T.SW = s.SW; T.n_tags = s.n_tags;
        *slot_serial = T.slot_serial = next_serial.fetch_add(1);
    }
    if (fields) {
        const TagFields& f = *fields;
        T.field_serial = 0;
        if ((rc = upload(e, T.field_rank, f.field_rank, what)) || (rc = upload(e, T.field_off, f.field_off, what)) ||
            (rc = upload(e, T.field_len, f.field_len, what)) || (rc = upload(e, T.valid, f.valid, what)) ||
            (rc = upload(e, T.field_blob, f.blob, what)))
            return rc;
        HIP_TRY(hipStreamSynchronize(e->stream), what);
        T.n_fields = f.n_fields;
        *field_serial = T.field_serial = next_serial.fetch_add(1);
    }
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

void tags_json_serials(gft_engine* e, uint64_t* slot_serial, uint64_t* field_serial) {
    if (slot_serial) *slot_serial = 0;
    if (field_serial) *field_serial = 0;
    if (!e) return;
    GFT_LOCK(e);
    if (slot_serial) *slot_serial = e->d_tagdoc.slot_serial;
    if (field_serial) *field_serial = e->d_tagdoc.field_serial;
}

int tags_json_device(gft_engine* e, const uint32_t* d_hit_bitmap, const uint32_t* d_leaf_field, const uint64_t* d_rec_off, uint64_t n_records,
                     uint64_t n_leaves, const uint64_t* d_hole_len, uint8_t* d_out, uint64_t cap, uint64_t* d_out_off, uint64_t* total) try {
    if (!e) return GFT_E_INVALID;
    GFT_LOCK(e);
    if (total) *total = 0;
    int rc = batch_checks(e, d_hit_bitmap, d_leaf_field, d_rec_off, n_records, n_leaves);
    if (rc) return rc;
    DeviceGuard g(e->device);
    e->d_tagdoc.staged = false;            // (the slot rows are this call's now)
    TagDocParams P{};
    if ((rc = slot_rows(e, P, d_hit_bitmap, d_leaf_field, n_leaves))) return rc;
    P.rec_off = d_rec_off; P.n_records = n_records; P.hole_len = d_hole_len;
    return tagdoc_text(e, P, d_out, cap, d_out_off, false, total);
} GFT_CATCH((e ? &e->err : nullptr))

int tags_json_stage(gft_engine* e, const uint32_t* d_hit_bitmap, const uint32_t* d_leaf_field, const uint64_t* d_rec_off, uint64_t n_records,
                    uint64_t n_leaves, const uint64_t** d_rec_off_kept) try {
    if (!e) return GFT_E_INVALID;
    GFT_LOCK(e);
    int rc = batch_checks(e, d_hit_bitmap, d_leaf_field, d_rec_off, n_records, n_leaves);
    if (rc) return rc;
    DeviceGuard g(e->device);
    auto& T = e->d_tagdoc;
    T.staged = false;
    if ((rc = room(e, T.leaf_field, n_leaves * 4, kTagDocRoom)) || (rc = room(e, T.rec_off, (n_records + 1) * 8, kTagDocRoom))) return rc;
    TagDocParams P{};
    if ((rc = slot_rows(e, P, d_hit_bitmap, d_leaf_field, n_leaves))) return rc;
    if (n_leaves) HIP_TRY(hipMemcpyAsync(T.leaf_field.p, d_leaf_field, n_leaves * 4, hipMemcpyDeviceToDevice, e->stream), "tag document");
    if (n_records) HIP_TRY(hipMemcpyAsync(T.rec_off.p, d_rec_off, (n_records + 1) * 8, hipMemcpyDeviceToDevice, e->stream), "tag document");
    HIP_TRY(hipStreamSynchronize(e->stream), "tag document");
    T.staged = true; T.staged_records = n_records; T.staged_leaves = n_leaves;
    if (d_rec_off_kept) *d_rec_off_kept = T.rec_off.as<uint64_t>();
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

int tags_json_owned(gft_engine* e, const uint64_t* h_hole_len, const uint8_t** d_text, const uint64_t** d_out_off, uint64_t* total) try {
    if (!e || !d_text || !d_out_off || !total) return GFT_E_INVALID;
    GFT_LOCK(e);
    int rc = tagdoc_entry_checks(e);
    if (rc) return rc;
    auto& T = e->d_tagdoc;
    if (!T.staged || !T.slot_serial || !T.field_serial) return fail(e, GFT_E_INVALID, "tag document: no batch staged");
    DeviceGuard g(e->device);
    const uint64_t n = T.staged_records;
    const uint64_t* d_hole_len = nullptr;
    if (h_hole_len && n) {
        SyncOnExit drain(e);
        if ((rc = room(e, T.hole_len, n * 8, kTagDocRoom))) return rc;
        HIP_TRY(hipMemcpyAsync(T.hole_len.p, h_hole_len, n * 8, hipMemcpyHostToDevice, e->stream), "hole lengths upload");
        HIP_TRY(hipStreamSynchronize(e->stream), "hole lengths upload");
        d_hole_len = T.hole_len.as<uint64_t>();
    }
    TagDocParams P{};
    table_params(T, P);
    P.slot_rows = T.slot_rows.as<uint32_t>(); P.leaf_field = T.leaf_field.as<uint32_t>(); P.rec_off = T.rec_off.as<uint64_t>();
    P.n_leaves = T.staged_leaves; P.n_records = n; P.hole_len = d_hole_len;
    // (the flag words still hold what the slot kernel found)
    uint8_t* out = nullptr;
    uint64_t* off = nullptr;
    if ((rc = tagdoc_text(e, P, out, 0, off, true, total))) return rc;
    *d_text = out; *d_out_off = off;
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

}  // namespace gft
