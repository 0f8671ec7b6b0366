// group_records.cpp -- the group finder's record route (rule_set.hpp, gft_rules.hip): a schema and what is compiled from it
// (Records), the one function that makes one, and a batch of (field, string) leaves through the finder and the two rule kernels
// -- or, for the tag calls (group_tags.cpp), the three tag kernels.
#include "group_records.hpp"

#include <set>

namespace gft {

GroupFinder::Records* GroupFinder::schema_records(const char* what, Error& err) {
    if (!rec_) err = std::string(what) + ": no schema set (gft_group_set_schema)";
    return rec_.get();
}

int GroupFinder::compile_set(Records& r, Error& err) {
    RuleSet fresh;
    int rc = compile_rules(rules_, findthem_->tags(), findthem_->tag_ids(), r.schema, r.inc, r.exc, fresh, err);
    if (rc) return rc;
    r.set = std::move(fresh);
    r.rules_version = rules_version_;
    r.n_exprs = findthem_->expressions().size();
    r.serial = 0;
    return GFT_OK;
}

int GroupFinder::make_records(const std::vector<std::string>& paths, const std::vector<std::string>& includePaths,
                              const std::vector<std::string>& excludePaths, Records& out, Error& err) {
    out.schema = paths; out.inc = includePaths; out.exc = excludePaths;
    int rc = compile_set(out, err);
    if (rc) return rc;
    out.json_rc = compile_json_schema(paths, out.json, out.json_err);
    return GFT_OK;
}

int GroupFinder::SetSchema(const std::vector<std::string>& paths, const std::vector<std::string>& includePaths,
                           const std::vector<std::string>& excludePaths, Error& err) {
    std::set<std::string> seen;
    for (const auto& p : paths)
        if (!seen.insert(p).second) { err = "record schema: field path '" + p + "' is listed twice"; return GFT_E_INVALID; }
    auto next = std::make_shared<Records>();
    int rc = make_records(paths, includePaths, excludePaths, *next, err);
    if (rc) return rc;
    rec_ = std::move(next);                // (a schema beyond the trie's limits stands: json_rc answers the JSON calls)
    return GFT_OK;
}

int GroupFinder::compile(Records& r, Error& err) {
    if (r.rules_version == rules_version_ && r.n_exprs == findthem_->expressions().size()) return GFT_OK;
    return compile_set(r, err);
}

int GroupFinder::install(gft_engine* e, Records& r, Error& err) {
    if (r.serial && rules_serial(e) == r.serial) return GFT_OK;
    int rc = rules_install(e, r.set, &r.serial);
    if (rc) { r.serial = 0; err = gft_last_error(e); }
    return rc;
}

int GroupFinder::DebugEvalRules(const uint32_t* hit_bitmap, uint32_t n_exprs, const uint32_t* leaf_field, const uint64_t* rec_off,
                                uint64_t n_records, uint64_t n_leaves, uint32_t* rule_bitmap, Error& err) {
    Records* r = schema_records("record batch", err);
    if (!r) return GFT_E_INVALID;
    int rc = compile(*r, err);
    if (rc) return rc;
    const RuleSet& rs = r->set;
    if (n_exprs != rs.n_exprs) { err = "gft_debug_eval_rules: n_exprs is not the finder's number of expressions"; return GFT_E_INVALID; }
    err = validate_records(rs.n_fields, leaf_field, rec_off, n_records, n_leaves);
    if (!err.empty()) return GFT_E_INVALID;
    if (!n_records || !rs.n_rules) return GFT_OK;
    if (!rule_bitmap || (n_leaves && n_exprs && !hit_bitmap)) { err = "gft_debug_eval_rules: null argument"; return GFT_E_INVALID; }
    eval_rules_host(rs, hit_bitmap, leaf_field, rec_off, n_records, rule_bitmap);
    return GFT_OK;
}

int GroupFinder::DebugEvalRulesDevice(const uint32_t* d_hit_bitmap, uint32_t n_exprs, const uint32_t* d_leaf_field, const uint64_t* d_rec_off,
                                      uint64_t n_records, uint64_t n_leaves, uint32_t* d_rule_bitmap, Error& err) {
    Records* r = schema_records("record batch", err);
    if (!r) return GFT_E_INVALID;
    int rc = compile(*r, err);
    if (rc) return rc;
    if (n_exprs != r->set.n_exprs) { err = "gft_debug_eval_rules_device: n_exprs is not the finder's number of expressions"; return GFT_E_INVALID; }
    gft_engine* e = findthem_->device_engine();
    if (!e) { err = "no GPU engine"; return GFT_E_HIP; }
    RulesLock whole_call(e);
    if ((rc = install(e, *r, err))) return rc;
    if ((rc = rules_eval_device(e, d_hit_bitmap, d_leaf_field, d_rec_off, n_records, n_leaves, d_rule_bitmap))) err = gft_last_error(e);
    return rc;
}

int GroupFinder::ProcessRecordsDevice(const uint8_t* d_text, const uint64_t* d_leaf_off, const uint32_t* d_leaf_field, const uint64_t* d_rec_off,
                                      uint64_t n_records, uint64_t n_leaves, uint32_t* d_rule_bitmap, Error& err) {
    Records* r = schema_records("record batch", err);
    RecordsOut out;
    out.d_rule_bitmap = d_rule_bitmap;
    return r ? records_device(*r, d_text, d_leaf_off, d_leaf_field, d_rec_off, n_records, n_leaves, out, err) : GFT_E_INVALID;
}

int GroupFinder::records_device(Records& r, const uint8_t* d_text, const uint64_t* d_leaf_off, const uint32_t* d_leaf_field, const uint64_t* d_rec_off,
                                uint64_t n_records, uint64_t n_leaves, const RecordsOut& out, Error& err) {
    int rc = compile(r, err);
    if (rc) return rc;
    if (!findthem_->device_resident_ok()) { err = "device-resident records need the GPU substring engine and no regex terms"; return GFT_E_UNSUPPORTED; }
    gft_engine* e = nullptr;
    if ((rc = single_device_engine(findthem_, "record batches", e, err))) return rc;
    // one state of the engine from the set's install to the read of the flags: another group on the same finder, called from
    // another thread, installs its own set and uses the same work buffers
    RulesLock whole_call(e);
    if ((rc = install(e, r, err))) return rc;
    const RuleSet& rs = r.set;
    uint32_t* d_hit = nullptr;
    if (n_leaves && rs.n_exprs) {
        if (!d_text || !d_leaf_off) { err = "record batch: null argument"; return GFT_E_INVALID; }
        if ((rc = rules_leaf_bitmap(e, n_leaves, (rs.n_exprs + 31) / 32, &d_hit))) { err = gft_last_error(e); return rc; }
        err = findthem_->ProcessDevice(d_text, d_leaf_off, n_leaves, d_hit);
        if (!err.empty()) return findthem_->last_code() ? findthem_->last_code() : GFT_E_ENGINE;
        // (the finder may have rebuilt its programs, never its expressions: the set installed above still fits)
    }
    if (out.tagdoc) {
        rc = tags_json_stage(e, d_hit, d_leaf_field, d_rec_off, n_records, n_leaves, &out.tagdoc->d_rec_off);
    } else if (out.owned) {
        rc = rules_tag_entries_owned(e, d_hit, d_leaf_field, d_rec_off, n_records, n_leaves, &out.owned->row_off, &out.owned->ent_field,
                                     &out.owned->ent_expr, &out.owned->total);
    } else if (out.d_entries) {
        const TagEntries& t = *out.d_entries;
        rc = rules_tag_entries_device(e, d_hit, d_leaf_field, d_rec_off, n_records, n_leaves, t.row_off, t.ent_field, t.ent_expr, t.ent_tag, t.cap,
                                      t.total);
    } else {
        rc = rules_eval_device(e, d_hit, d_leaf_field, d_rec_off, n_records, n_leaves, out.d_rule_bitmap);
    }
    if (rc) err = gft_last_error(e);
    return rc;
}

int GroupFinder::ProcessRecords(const uint8_t* text, const uint64_t* leaf_off, const uint32_t* leaf_field, const uint64_t* rec_off,
                                uint64_t n_records, uint64_t n_leaves, uint32_t* rule_bitmap, Error& err) {
    Records* r = schema_records("record batch", err);
    if (!r) return GFT_E_INVALID;
    int rc = compile(*r, err);
    if (rc) return rc;
    const RuleSet& rs = r->set;
    err = validate_records(rs.n_fields, leaf_field, rec_off, n_records, n_leaves);
    if (!err.empty()) return GFT_E_INVALID;
    if (n_leaves && (!text || !leaf_off)) { err = "record batch: null argument"; return GFT_E_INVALID; }
    for (uint64_t l = 0; l < n_leaves; l++)
        if (leaf_off[l] > leaf_off[l + 1]) { err = "record batch: leaf_off descends at leaf " + std::to_string(l); return GFT_E_INVALID; }
    const uint64_t RW = r->row_words(), EW = (rs.n_exprs + 31) / 32;
    if (!n_records || !RW) return GFT_OK;
    if (!rule_bitmap) { err = "record batch: null argument"; return GFT_E_INVALID; }
    gft_engine* e = nullptr;
    if ((rc = single_device_engine(findthem_, "record batches", e, err))) return rc;
    RulesLock whole_call(e);              // (staging buffers, set and work buffers: see ProcessRecordsDevice)
    static const uint64_t none = 0;
    void* d[5] = {};
    if (findthem_->device_resident_ok()) {
        const uint64_t text_bytes = n_leaves ? leaf_off[n_leaves] : 0;
        const void* src[5] = {text, n_leaves ? (const void*)leaf_off : &none, leaf_field, rec_off, nullptr};
        const uint64_t bytes[5] = {text_bytes, (n_leaves + 1) * 8, n_leaves * 4, (n_records + 1) * 8, 0};
        const uint64_t slack[5] = {64, 0, 0, 0, n_records * RW * 4};
        if ((rc = rules_stage(e, 5, src, bytes, slack, d))) { err = gft_last_error(e); return rc; }
        RecordsOut rows;
        rows.d_rule_bitmap = (uint32_t*)d[4];
        rc = records_device(*r, (const uint8_t*)d[0], (const uint64_t*)d[1], (const uint32_t*)d[2], (const uint64_t*)d[3], n_records, n_leaves, rows,
                            err);
        if (rc) return rc;
    } else {
        // regex terms, the prefilter, injected engines: the finder's own batch path gives the leaf bitmap
        std::vector<uint32_t> hit((size_t)(n_leaves * EW) + 1, 0);
        if (n_leaves && EW) {
            err = findthem_->ProcessTexts(text, leaf_off, n_leaves, hit.data());
            if (!err.empty()) return findthem_->last_code() ? findthem_->last_code() : GFT_E_ENGINE;
        }
        if ((rc = install(e, *r, err))) return rc;
        const void* src[4] = {hit.data(), leaf_field, rec_off, nullptr};
        const uint64_t bytes[4] = {n_leaves * EW * 4, n_leaves * 4, (n_records + 1) * 8, 0};
        const uint64_t slack[4] = {0, 0, 0, n_records * RW * 4};
        if ((rc = rules_stage(e, 4, src, bytes, slack, d))) { err = gft_last_error(e); return rc; }
        if ((rc = rules_eval_device(e, (const uint32_t*)d[0], (const uint32_t*)d[1], (const uint64_t*)d[2], n_records, n_leaves, (uint32_t*)d[3]))) {
            err = gft_last_error(e);
            return rc;
        }
        d[4] = d[3];
    }
    if ((rc = rules_fetch(e, rule_bitmap, d[4], n_records * RW * 4))) err = gft_last_error(e);
    return rc;
}

}  // namespace gft
