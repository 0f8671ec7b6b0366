// group_tags.cpp -- the group finder's tag calls on the device: TagObject's map of every record of a batch as a sparse list of
// (field, expression) entries (gft_tags.hpp, tag_entries.hpp).  The record and JSON routes are those of group_records.cpp and
// group_json.cpp, asked for entries instead of rule rows.
#include <algorithm>

#include "group_records.hpp"
#include "tag_entries.hpp"

namespace gft {

namespace {
const char* entries_args(const GroupFinder::TagEntries& t) {
    if (!t.row_off) return "tag entries: no row_off";
    if (t.cap && (!t.ent_field || !t.ent_expr)) return "tag entries: a cap but no array";
    return nullptr;
}
}  // namespace

int GroupFinder::TagRecordsDevice(const uint8_t* d_text, const uint64_t* d_leaf_off, const uint32_t* d_leaf_field, const uint64_t* d_rec_off,
                                  uint64_t n_records, uint64_t n_leaves, const TagEntries& d_out, Error& err) {
    Records* r = schema_records("record batch", err);
    if (!r) return GFT_E_INVALID;
    if (const char* why = entries_args(d_out)) { err = why; return GFT_E_INVALID; }
    RecordsOut out;
    out.d_entries = &d_out;
    return records_device(*r, d_text, d_leaf_off, d_leaf_field, d_rec_off, n_records, n_leaves, out, err);
}

int GroupFinder::TagJsonsDevice(const uint8_t* d_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint8_t* d_status, const TagEntries& d_out,
                                Error& err) {
    Records* r = schema_records("JSON batch", err);
    if (!r) return GFT_E_INVALID;
    if (const char* why = entries_args(d_out)) { err = why; return GFT_E_INVALID; }
    RecordsOut out;
    out.d_entries = &d_out;
    return jsons_device(*r, d_blob, d_doc_off, n_docs, d_status, out, err);
}

int GroupFinder::TagRecords(const uint8_t* text, const uint64_t* leaf_off, const uint32_t* leaf_field, const uint64_t* rec_off, uint64_t n_records,
                            uint64_t n_leaves, const TagEntries& out, Error& err) {
    Records* r = schema_records("record batch", err);
    if (!r) return GFT_E_INVALID;
    int rc = compile(*r, err);
    if (rc) return rc;
    const RuleSet& rs = r->set;
    err = validate_records(rs.n_fields, leaf_field, rec_off, n_records, n_leaves);
    if (!err.empty()) return GFT_E_INVALID;
    if (const char* why = entries_args(out)) { err = why; return GFT_E_INVALID; }
    if (n_leaves && (!text || !leaf_off)) { err = "record batch: null argument"; return GFT_E_INVALID; }
    for (uint64_t l = 0; l < n_leaves; l++)
        if (leaf_off[l] > leaf_off[l + 1]) { err = "record batch: leaf_off descends at leaf " + std::to_string(l); return GFT_E_INVALID; }
    if (out.total) *out.total = 0;
    if (!n_records) { out.row_off[0] = 0; return GFT_OK; }
    gft_engine* e = findthem_->device_engine();
    if (e && findthem_->device_resident_ok() && gft_n_devices(e) == 1) {
        RulesLock whole_call(e);          // (staging buffers, set and work buffers: see ProcessRecordsDevice)
        static const uint64_t none = 0;
        void* d[4] = {};
        const uint64_t text_bytes = n_leaves ? leaf_off[n_leaves] : 0;
        const void* src[4] = {text, n_leaves ? (const void*)leaf_off : &none, leaf_field, rec_off};
        const uint64_t bytes[4] = {text_bytes, (n_leaves + 1) * 8, n_leaves * 4, (n_records + 1) * 8};
        const uint64_t slack[4] = {64, 0, 0, 0};
        if ((rc = rules_stage(e, 4, src, bytes, slack, d))) { err = gft_last_error(e); return rc; }
        RecordsOut dev;
        RecordsOut::Owned own;
        dev.owned = &own;
        rc = records_device(*r, (const uint8_t*)d[0], (const uint64_t*)d[1], (const uint32_t*)d[2], (const uint64_t*)d[3], n_records, n_leaves, dev, err);
        if (rc) return rc;
        // the sparse result down: the offsets, and the entries that fit the caller's arrays
        const uint64_t n = std::min(own.total, out.cap);
        if ((rc = rules_fetch(e, out.row_off, own.row_off, (n_records + 1) * 8)) || (rc = rules_fetch(e, out.ent_field, own.ent_field, n * 4)) ||
            (rc = rules_fetch(e, out.ent_expr, own.ent_expr, n * 4))) {
            err = gft_last_error(e);
            return rc;
        }
        if (out.ent_tag)
            for (uint64_t k = 0; k < n; k++) out.ent_tag[k] = rs.expr_tag[out.ent_expr[k]];
        if (out.total) *out.total = own.total;
        return GFT_OK;
    }
    // regex terms, the prefilter, injected engines, several devices: the finder's own batch path gives the leaf bitmap
    const uint64_t EW = (rs.n_exprs + 31) / 32;
    std::vector<uint32_t> hit((size_t)(n_leaves * EW) + 1, 0);
    if (n_leaves && EW) {
        err = findthem_->ProcessTexts(text, leaf_off, n_leaves, hit.data());
        if (!err.empty()) return findthem_->last_code() ? findthem_->last_code() : GFT_E_ENGINE;
    }
    tag_entries_host(rs, hit.data(), rs.n_exprs, leaf_field, rec_off, n_records, n_leaves, out.row_off, out.ent_field, out.ent_expr, out.ent_tag,
                     out.cap, out.total);
    return GFT_OK;
}

int GroupFinder::TagJsonsSchema(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, std::vector<DocResult>& out, Error& err) {
    return jsons_schema(blob, doc_off, n_docs, true, out, err);
}

int GroupFinder::TagJsonsAuto(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const std::vector<std::string>& includePaths,
                              const std::vector<std::string>& excludePaths, std::vector<DocResult>& out, Error& err) {
    return jsons_auto(blob, doc_off, n_docs, includePaths, excludePaths, true, out, err);
}

int GroupFinder::DebugTagEntries(const uint32_t* hit_bitmap, uint32_t n_exprs, const uint32_t* leaf_field, const uint64_t* rec_off,
                                 uint64_t n_records, uint64_t n_leaves, const TagEntries& out, Error& err) {
    Records* r = schema_records("record batch", err);
    if (!r) return GFT_E_INVALID;
    int rc = compile(*r, err);
    if (rc) return rc;
    const RuleSet& rs = r->set;
    if (n_exprs != rs.n_exprs) { err = "gft_debug_tag_entries: n_exprs is not the finder's number of expressions"; return GFT_E_INVALID; }
    err = validate_records(rs.n_fields, leaf_field, rec_off, n_records, n_leaves);
    if (!err.empty()) return GFT_E_INVALID;
    if (const char* why = entries_args(out)) { err = why; return GFT_E_INVALID; }
    if (n_leaves && n_exprs && !hit_bitmap) { err = "gft_debug_tag_entries: null argument"; return GFT_E_INVALID; }
    tag_entries_host(rs, hit_bitmap, n_exprs, leaf_field, rec_off, n_records, n_leaves, out.row_off, out.ent_field, out.ent_expr, out.ent_tag, out.cap,
                     out.total);
    return GFT_OK;
}

int GroupFinder::DebugTagEntriesDevice(const uint32_t* d_hit_bitmap, uint32_t n_exprs, const uint32_t* d_leaf_field, const uint64_t* d_rec_off,
                                       uint64_t n_records, uint64_t n_leaves, const TagEntries& d_out, Error& err) {
    Records* r = schema_records("record batch", err);
    if (!r) return GFT_E_INVALID;
    int rc = compile(*r, err);
    if (rc) return rc;
    if (n_exprs != r->set.n_exprs) { err = "gft_debug_tag_entries_device: n_exprs is not the finder's number of expressions"; return GFT_E_INVALID; }
    gft_engine* e = findthem_->device_engine();
    if (!e) { err = "no GPU engine"; return GFT_E_HIP; }
    RulesLock whole_call(e);
    if ((rc = install(e, *r, err))) return rc;
    if ((rc = rules_tag_entries_device(e, d_hit_bitmap, d_leaf_field, d_rec_off, n_records, n_leaves, d_out.row_off, d_out.ent_field, d_out.ent_expr,
                                       d_out.ent_tag, d_out.cap, d_out.total)))
        err = gft_last_error(e);
    return rc;
}

}  // namespace gft
