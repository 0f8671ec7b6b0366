// group_tags.cpp -- the group finder's tag calls on the device: TagObject's map of every record of a batch as a sparse list of
// (field, expression) entries (gft_tags.hpp, tag_entries.hpp).  The record and JSON routes are those of group_records.cpp and
// group_json.cpp, asked for entries instead of rule rows.
#include <algorithm>
#include <cstring>

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

int GroupFinder::TagJsonsSchema(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, std::vector<DocResult>& out, Error& err,
                                ResultText* text) {
    return jsons_schema(blob, doc_off, n_docs, true, out, err, text);
}

int GroupFinder::TagJsonsAuto(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const std::vector<std::string>& includePaths,
                              const std::vector<std::string>& excludePaths, std::vector<DocResult>& out, Error& err, ResultText* text) {
    return jsons_auto(blob, doc_off, n_docs, includePaths, excludePaths, true, out, err, text);
}

// ---- the tag result document written on the device ------------------------------------------------------------------------------
const TagSlots* GroupFinder::tag_slots() {
    const auto& exprs = findthem_->expressions();
    if (tslots_n_exprs_ != exprs.size()) {
        std::vector<TagExpr> list;
        for (const auto& x : exprs) list.push_back({&x.tag, &x.exprString});
        auto next = std::make_shared<TagSlots>();
        tslots_why_.clear();
        tslots_ = make_tag_slots(list, *next, tslots_why_) ? std::move(next) : nullptr;
        tslots_n_exprs_ = exprs.size();
        tslots_serial_ = 0;
    }
    return tslots_.get();
}

const TagFields* GroupFinder::tag_fields(Records& r) {
    if (!r.tfields_made) {
        auto next = std::make_shared<TagFields>();
        r.tfields = make_tag_fields(r.schema, r.set.valid, *next, r.tfields_why) ? std::move(next) : nullptr;
        r.tfields_made = true;
        r.tfields_serial = 0;
    }
    return r.tfields.get();
}

int GroupFinder::tagdoc_ready(gft_engine* e, Records& r, Error& err) {
    const TagSlots* ts = tag_slots();
    if (!ts) { err = "tag document: " + tslots_why_; return GFT_E_UNSUPPORTED; }
    const TagFields* tf = tag_fields(r);
    if (!tf) { err = "tag document: " + r.tfields_why; return GFT_E_UNSUPPORTED; }
    if (!e) return GFT_OK;
    uint64_t on_slots = 0, on_fields = 0;
    tags_json_serials(e, &on_slots, &on_fields);
    const bool slots_there = tslots_serial_ && on_slots == tslots_serial_, fields_there = r.tfields_serial && on_fields == r.tfields_serial;
    if (slots_there && fields_there) return GFT_OK;
    int rc = tags_json_install(e, slots_there ? nullptr : ts, &tslots_serial_, fields_there ? nullptr : tf, &r.tfields_serial);
    if (rc) { tslots_serial_ = r.tfields_serial = 0; err = gft_last_error(e); }
    return rc;
}

int GroupFinder::TagsJsonDevice(const uint32_t* d_hit_bitmap, const uint32_t* d_leaf_field, const uint64_t* d_rec_off, uint64_t n_records,
                                uint64_t n_leaves, const uint64_t* d_hole_len, uint8_t* d_out, uint64_t cap, uint64_t* d_out_off, uint64_t* total,
                                Error& err) {
    Records* r = schema_records("tag document", err);
    if (!r) return GFT_E_INVALID;
    int rc = compile(*r, err);
    if (rc) return rc;
    gft_engine* e = nullptr;
    if ((rc = single_device_engine(findthem_, "tag documents", e, err))) return rc;
    RulesLock whole_call(e);               // (another group on the same finder installs its own tables)
    if ((rc = tagdoc_ready(e, *r, err))) return rc;
    if ((rc = tags_json_device(e, d_hit_bitmap, d_leaf_field, d_rec_off, n_records, n_leaves, d_hole_len, d_out, cap, d_out_off, total)))
        err = gft_last_error(e);
    return rc;
}

int GroupFinder::DebugTagsJson(const uint32_t* hit_bitmap, uint32_t n_exprs, const uint32_t* leaf_field, const uint64_t* rec_off, uint64_t n_records,
                               uint64_t n_leaves, const uint64_t* hole_len, uint8_t* out, uint64_t cap, uint64_t* out_off, uint64_t* total,
                               Error& err) {
    Records* r = schema_records("tag document", err);
    if (!r) return GFT_E_INVALID;
    int rc = compile(*r, err);
    if (rc) return rc;
    if (n_exprs != findthem_->expressions().size()) { err = "gft_debug_tags_json: n_exprs is not the finder's number of expressions"; return GFT_E_INVALID; }
    err = validate_records(r->set.n_fields, leaf_field, rec_off, n_records, n_leaves);
    if (!err.empty()) return GFT_E_INVALID;
    if (!out_off || (cap && !out) || (n_leaves && n_exprs && !hit_bitmap)) { err = "gft_debug_tags_json: null argument"; return GFT_E_INVALID; }
    if ((rc = tagdoc_ready(nullptr, *r, err))) return rc;
    const int refusal = tags_json_host(*tslots_, *r->tfields, hit_bitmap, leaf_field, rec_off, n_records, hole_len, out, cap, out_off, total);
    if (!refusal) return GFT_OK;
    err = std::string("gft_debug_tags_json: ") + tags_json_refusal_text(refusal);
    return refusal == kTagsJsonHole ? GFT_E_INVALID : GFT_E_UNSUPPORTED;
}

int GroupFinder::json_tag_text(gft_engine* e, Records& r, const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const uint8_t* d_blob,
                               const uint64_t* d_doc_off, uint8_t* d_status, std::string& text, Error& err) {
    int rc = tagdoc_ready(e, r, err);
    if (rc) return rc;
    // the leaves through the finder, then the slot rows, the leaf fields and the record offsets into the tag document's own
    // buffers: what the count and the fill read survives the finder calls of the host sub-batch below
    RecordsOut out;
    RecordsOut::TagDoc kept;
    out.tagdoc = &kept;
    if ((rc = jsons_device(r, d_blob, d_doc_off, n_docs, d_status, out, err))) return rc;
    std::vector<uint8_t> status(n_docs, 0);
    std::vector<uint64_t> rec_off(n_docs + 1, 0);
    if ((rc = rules_fetch(e, status.data(), d_status, n_docs)) || (rc = rules_fetch(e, rec_off.data(), kept.d_rec_off, (n_docs + 1) * 8))) {
        err = gft_last_error(e);
        return rc;
    }
    // what the device did not decide, and what is wider than a wave ranks: one sub-batch through the host route, every document
    // to its final text
    std::vector<uint8_t> by_host(status);
    uint64_t undecided = 0;
    for (uint64_t d = 0; d < n_docs; d++) {
        undecided += status[d] != 0;
        if (!status[d] && rec_off[d + 1] - rec_off[d] > GFT_TAGS_JSON_MAX_LEAVES) by_host[d] = 0xFF;
    }
    std::vector<uint64_t> host_docs;
    std::vector<DocResult> res;
    if ((rc = json_host_docs(r, blob, doc_off, n_docs, by_host, true, host_docs, res, err))) return rc;
    json_last_host = undecided;            // (a wide document was decided on the device: only its text is the host's)
    json_last_device = n_docs - undecided;
    std::vector<std::string> hole_text(host_docs.size());
    std::vector<uint64_t> hole_len;
    if (!host_docs.empty()) {
        hole_len.assign(n_docs, 0);
        for (size_t k = 0; k < host_docs.size(); k++) {
            tag_doc_text(res[k].err, res[k].tags, hole_text[k]);
            hole_len[host_docs[k]] = hole_text[k].size();
        }
    }
    const uint8_t* d_text = nullptr; const uint64_t* d_out_off = nullptr;
    uint64_t total = 0;
    if ((rc = tags_json_owned(e, hole_len.empty() ? nullptr : hole_len.data(), &d_text, &d_out_off, &total))) {
        err = gft_last_error(e);
        return rc;
    }
    text.resize((size_t)total);
    if ((rc = rules_fetch(e, &text[0], d_text, total))) { err = gft_last_error(e); return rc; }
    if (!host_docs.empty()) {
        std::vector<uint64_t> out_off(n_docs + 1, 0);
        if ((rc = rules_fetch(e, out_off.data(), d_out_off, (n_docs + 1) * 8))) { err = gft_last_error(e); return rc; }
        for (size_t k = 0; k < host_docs.size(); k++) memcpy(&text[(size_t)out_off[host_docs[k]]], hole_text[k].data(), hole_text[k].size());
    }
    return GFT_OK;
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
