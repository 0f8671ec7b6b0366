// group_json.cpp -- the group finder's JSON routes on the device (json_schema.hpp, gft_json.hip): documents decoded into the
// record form against a schema's trie and sent down the record route (group_records.cpp), for the schema of SetSchema and for
// the one discovered from the batch (json_paths.hpp: k_json_paths).
#include <cstdlib>
#include <cstring>
#include <set>

#include "gft_result.hpp"
#include "gft_split.hpp"
#include "group_records.hpp"
#include "host_parallel.hpp"
#include "json_paths.hpp"
#include "rules_json.hpp"

namespace gft {

int GroupFinder::json_ready(gft_engine* e, Records& r, Error& err) {
    if (r.json_rc) { err = r.json_err; return r.json_rc; }
    if (!e || (r.json_serial && json_serial(e) == r.json_serial)) return GFT_OK;
    int rc = json_install(e, r.json, &r.json_serial);
    if (rc) { r.json_serial = 0; err = gft_last_error(e); }
    return rc;
}

int GroupFinder::JsonLeavesDevice(const uint8_t* d_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint8_t* d_status, uint64_t* d_rec_off,
                                  uint32_t* d_leaf_field, uint64_t* d_leaf_off, uint64_t leaf_cap, uint8_t* d_text, uint64_t text_cap,
                                  uint64_t* totals, Error& err) {
    Records* r = schema_records("JSON batch", err);
    if (!r) return GFT_E_INVALID;
    int rc = json_ready(nullptr, *r, err);
    if (rc) return rc;
    gft_engine* e = nullptr;
    if ((rc = single_device_engine(findthem_, "JSON batches", e, err))) return rc;
    RulesLock whole_call(e);               // (another group on the same finder installs its own trie)
    if ((rc = json_ready(e, *r, err))) return rc;
    if ((rc = json_leaves_device(e, d_blob, d_doc_off, n_docs, d_status, d_rec_off, d_leaf_field, d_leaf_off, leaf_cap, d_text, text_cap, totals)))
        err = gft_last_error(e);
    return rc;
}

int GroupFinder::ProcessJsonsDevice(const uint8_t* d_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint8_t* d_status, uint32_t* d_rule_bitmap,
                                    Error& err) {
    Records* r = schema_records("JSON batch", err);
    RecordsOut out;
    out.d_rule_bitmap = d_rule_bitmap;
    return r ? jsons_device(*r, d_blob, d_doc_off, n_docs, d_status, out, err) : GFT_E_INVALID;
}

int GroupFinder::jsons_device(Records& r, const uint8_t* d_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint8_t* d_status,
                              const RecordsOut& out, Error& err) {
    int rc = json_ready(nullptr, r, err);
    if (rc) return rc;
    if ((rc = compile(r, err))) return rc;
    if (!findthem_->device_resident_ok()) { err = "device-resident JSON batches need the GPU substring engine and no regex terms"; return GFT_E_UNSUPPORTED; }
    gft_engine* e = nullptr;
    if ((rc = single_device_engine(findthem_, "JSON batches", e, err))) return rc;
    RulesLock whole_call(e);
    if ((rc = json_ready(e, r, err))) return rc;
    const uint64_t* d_rec_off = nullptr; const uint32_t* d_leaf_field = nullptr; const uint64_t* d_leaf_off = nullptr; const uint8_t* d_text = nullptr;
    uint64_t totals[2] = {0, 0};
    if ((rc = json_leaves_owned(e, d_blob, d_doc_off, n_docs, d_status, &d_rec_off, &d_leaf_field, &d_leaf_off, &d_text, totals))) {
        err = gft_last_error(e);
        return rc;
    }
    last_leaves = totals[0];
    last_bytes = totals[1];
    return records_device(r, d_text, d_leaf_off, d_leaf_field, d_rec_off, n_docs, totals[0], out, err);
}

int GroupFinder::json_staged(gft_engine* e, Records& r, const uint8_t* d_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint8_t* d_status,
                             uint32_t* d_rows, bool want_tags, JsonStaged& s, Error& err, bool fetch_rows) {
    s.status.assign(n_docs, 0);
    RecordsOut out;
    RecordsOut::Owned own;
    const uint64_t RW = r.row_words();
    if (want_tags) {
        out.owned = &own;
    } else {
        if (fetch_rows) s.rows.assign((size_t)(n_docs * RW) + 1, 0);
        out.d_rule_bitmap = d_rows;
    }
    int rc = jsons_device(r, d_blob, d_doc_off, n_docs, d_status, out, err);
    if (rc) return rc;
    if ((rc = rules_fetch(e, s.status.data(), d_status, n_docs))) { err = gft_last_error(e); return rc; }
    if (want_tags) {
        // only the sparse result crosses the link: the offsets and the two entry columns (the tag is the expression's)
        s.row_off.assign(n_docs + 1, 0);
        s.ent_field.assign((size_t)own.total + 1, 0);
        s.ent_expr.assign((size_t)own.total + 1, 0);
        if ((rc = rules_fetch(e, s.row_off.data(), own.row_off, (n_docs + 1) * 8)) || (rc = rules_fetch(e, s.ent_field.data(), own.ent_field, own.total * 4)) ||
            (rc = rules_fetch(e, s.ent_expr.data(), own.ent_expr, own.total * 4)))
            err = gft_last_error(e);
    } else if (fetch_rows && (rc = rules_fetch(e, s.rows.data(), d_rows, n_docs * RW * 4))) {
        err = gft_last_error(e);
    }
    return rc;
}

int GroupFinder::json_host_docs(const Records& r, const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const std::vector<uint8_t>& status,
                                bool want_tags, std::vector<uint64_t>& host_docs, std::vector<DocResult>& res, Error& err) {
    host_docs.clear();
    res.clear();
    for (uint64_t d = 0; d < n_docs; d++)
        if (status[d]) host_docs.push_back(d);
    if (!host_docs.empty()) {
        std::vector<uint64_t> off(host_docs.size() + 1, 0);
        for (size_t k = 0; k < host_docs.size(); k++) off[k + 1] = off[k] + (doc_off[host_docs[k] + 1] - doc_off[host_docs[k]]);
        std::vector<uint8_t> sub(off.back() + 64, 0);
        for (size_t k = 0; k < host_docs.size(); k++) memcpy(sub.data() + off[k], blob + doc_off[host_docs[k]], (size_t)(off[k + 1] - off[k]));
        err = ProcessJsons(sub.data(), off.data(), host_docs.size(), r.inc, r.exc, want_tags, res);
        if (!err.empty()) return GFT_E_ENGINE;
    }
    json_last_host = host_docs.size();
    json_last_device = n_docs - host_docs.size();
    return GFT_OK;
}

int GroupFinder::json_results(const Records& r, const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const JsonStaged& s, bool want_tags,
                              std::vector<DocResult>& out, Error& err) {
    const uint64_t RW = r.row_words();
    const std::vector<uint8_t>& status = s.status;
    // what the device did not decide: one sub-batch through the host route
    std::vector<uint64_t> host_docs;
    std::vector<DocResult> res;
    int rc = json_host_docs(r, blob, doc_off, n_docs, status, want_tags, host_docs, res, err);
    if (rc) return rc;
    for (size_t k = 0; k < host_docs.size(); k++) out[host_docs[k]] = std::move(res[k]);
    if (want_tags) {
        // a document's entries -> its tag map; the set's insert drops what a repeated field says twice
        const auto& exprs = findthem_->expressions();
        parallel_for(n_docs, [&](uint64_t d, unsigned) {
            if (status[d]) return;
            for (uint64_t k = s.row_off[d]; k < s.row_off[d + 1]; k++) {
                const auto& x = exprs[s.ent_expr[k]];
                out[d].tags[x.tag][r.schema[s.ent_field[k]]].insert(x.exprString);
            }
        });
        return GFT_OK;
    }
    const std::vector<uint32_t>& rows = s.rows;
    const auto& names = RuleExprs();
    parallel_for(n_docs, [&](uint64_t d, unsigned) {
        if (status[d]) return;
        const uint32_t* row = rows.data() + d * RW;
        for (uint32_t w = 0; w < RW; w++)
            for (uint32_t bits = row[w]; bits; bits &= bits - 1) {
                const RuleExpr& re = names[w * 32 + (uint32_t)__builtin_ctz(bits)];
                out[d].rules[*re.name].push_back(*re.expr);
            }
    });
    return GFT_OK;
}

// ---- the result document written on the device ----------------------------------------------------------------------------------
bool GroupFinder::env_device_result() {
    const char* v = getenv("GFT_DEVICE_RESULT");
    return !(v && v[0] == '0' && !v[1]);
}

const RuleFragments* GroupFinder::fragments() {
    if (frags_version_ != rules_version_) {
        auto next = std::make_shared<RuleFragments>();
        frags_why_.clear();
        frags_ = make_rule_fragments(RuleExprs(), *next, frags_why_) ? std::move(next) : nullptr;
        frags_version_ = rules_version_;
        frags_serial_ = 0;
    }
    return frags_.get();
}

int GroupFinder::result_ready(gft_engine* e, Error& err) {
    const RuleFragments* fr = fragments();
    if (!fr) { err = "result document: " + frags_why_; return GFT_E_UNSUPPORTED; }
    if (frags_serial_ && rules_json_serial(e) == frags_serial_) return GFT_OK;
    int rc = rules_json_install(e, *fr, &frags_serial_);
    if (rc) { frags_serial_ = 0; err = gft_last_error(e); }
    return rc;
}

int GroupFinder::RulesJsonDevice(const uint32_t* d_rule_bitmap, uint64_t n_docs, const uint64_t* d_hole_len, uint8_t* d_out, uint64_t cap,
                                 uint64_t* d_out_off, uint64_t* total, Error& err) {
    gft_engine* e = nullptr;
    int rc = single_device_engine(findthem_, "result documents", e, err);
    if (rc) return rc;
    RulesLock whole_call(e);               // (another group on the same finder installs its own table)
    if ((rc = result_ready(e, err))) return rc;
    if ((rc = rules_json_device(e, d_rule_bitmap, n_docs, d_hole_len, d_out, cap, d_out_off, total))) err = gft_last_error(e);
    return rc;
}

int GroupFinder::DebugRulesJson(const uint32_t* rule_bitmap, uint64_t n_docs, const uint64_t* hole_len, uint8_t* out, uint64_t cap,
                                uint64_t* out_off, uint64_t* total, Error& err) {
    const RuleFragments* fr = fragments();
    if (!fr) { err = "gft_debug_rules_json: " + frags_why_; return GFT_E_UNSUPPORTED; }
    if (!out_off || (cap && !out) || (n_docs && fr->n_exprs() && !rule_bitmap)) { err = "gft_debug_rules_json: null argument"; return GFT_E_INVALID; }
    if (!rules_json_host(*fr, rule_bitmap, n_docs, hole_len, out, cap, out_off, total)) { err = "gft_debug_rules_json: a hole of 4 GiB or more"; return GFT_E_INVALID; }
    return GFT_OK;
}

int GroupFinder::json_text(gft_engine* e, const Records& r, const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const uint32_t* d_rows,
                           const JsonStaged& s, std::string& text, Error& err) {
    // what the device did not decide: one sub-batch through the host route, every document to its final text
    std::vector<uint64_t> host_docs;
    std::vector<DocResult> res;
    int rc = json_host_docs(r, blob, doc_off, n_docs, s.status, false, host_docs, res, err);
    if (rc) return rc;
    std::vector<std::string> hole_text(host_docs.size());
    std::vector<uint64_t> hole_len;
    if (!host_docs.empty()) {
        hole_len.assign(n_docs, 0);
        for (size_t k = 0; k < host_docs.size(); k++) {
            rule_doc_text(res[k].err, res[k].rules, hole_text[k]);
            hole_len[host_docs[k]] = hole_text[k].size();
        }
    }
    const uint8_t* d_text = nullptr; const uint64_t* d_out_off = nullptr;
    uint64_t total = 0;
    if ((rc = rules_json_owned(e, d_rows, n_docs, hole_len.empty() ? nullptr : hole_len.data(), &d_text, &d_out_off, &total))) {
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

int GroupFinder::json_batch(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const std::vector<std::string>& includePaths,
                            const std::vector<std::string>& excludePaths, bool want_tags, uint64_t row_words, const ChooseRecords& choose,
                            std::vector<DocResult>& out, Error& err, ResultText* text, JsonLines* lines) {
    gft_engine* e = findthem_->device_engine();
    json_last_device = json_last_host = 0;
    auto by_host = [&]() -> int {
        if (lines && lines->off.empty()) {     // (not split on the device: the kernels' walk on the host)
            uint64_t n = 0;
            int rc = split_lines_host(blob, lines->len, GFT_SPLIT_JSON_LINES, nullptr, 0, &n);
            lines->off.assign(n + 1, 0);
            if (!rc) rc = split_lines_host(blob, lines->len, GFT_SPLIT_JSON_LINES, lines->off.data(), n + 1, &n);
            if (rc) { err = "JSON Lines: the blob could not be split"; return rc; }
            doc_off = lines->off.data();
            n_docs = n;
            if ((rc = json_check_offsets(doc_off, n_docs, err))) return rc;
        }
        err = ProcessJsons(blob, doc_off, n_docs, includePaths, excludePaths, want_tags, out);
        json_last_host = n_docs;
        return err.empty() ? GFT_OK : GFT_E_ENGINE;
    };
    // regex terms, injected engines, several devices: the walk on host threads, for every document
    if (!e || !findthem_->device_resident_ok() || gft_n_devices(e) != 1) return by_host();
    out.assign(n_docs, DocResult());
    if (!n_docs && !(lines && lines->len)) return GFT_OK;
    JsonStaged staged;
    std::shared_ptr<Records> r;            // (held to the end: the call's own, whatever becomes of the member it came from)
    {
        RulesLock whole_call(e);           // (the staging buffers, from the upload to the read of the rows)
        const uint8_t* d_blob = nullptr; const uint64_t* d_doc_off = nullptr; uint8_t* d_status = nullptr; uint32_t* d_rows = nullptr;
        int rc = lines ? json_stage_lines(e, blob, lines->len, want_tags ? 0 : row_words * 4, &d_blob, &d_doc_off, &d_status, &d_rows, lines->off)
                       : json_stage(e, blob, doc_off, n_docs, want_tags ? 0 : row_words * 4, &d_blob, &d_doc_off, &d_status, &d_rows);
        if (rc) { err = gft_last_error(e); return rc; }
        if (lines) {                           // the batch's shape is known only now
            doc_off = lines->off.data();
            n_docs = lines->off.size() - 1;
            out.assign(n_docs, DocResult());
            if (!n_docs) return GFT_OK;
        }
        r = choose(e, d_blob, d_doc_off, n_docs, rc);
        if (rc) return rc;
        // the document from the rows where they are, unless the table was refused (the host serialisation is the route then)
        const bool on_device = r && text && text->text && !want_tags && device_result_ && fragments();
        if (on_device) {
            if ((rc = result_ready(e, err))) return rc;
            if ((rc = json_staged(e, *r, d_blob, d_doc_off, n_docs, d_status, d_rows, false, staged, err, false))) return rc;
            if ((rc = json_text(e, *r, blob, doc_off, n_docs, d_rows, staged, *text->text, err))) return rc;
            text->written = true;
            out.clear();
            return GFT_OK;
        }
        // the tag document from the leaf rows where they are, unless a table was refused.  A batch the contract refuses, or a
        // text the device has no room for, takes the entries route below: a call that succeeds there never fails here
        if (r && text && text->text && want_tags && device_result_) {
            if (!(rc = tagdoc_ready(nullptr, *r, err))) rc = json_tag_text(e, *r, blob, doc_off, n_docs, d_blob, d_doc_off, d_status, *text->text, err);
            if (!rc) {
                text->written = true;
                out.clear();
                return GFT_OK;
            }
            if (rc != GFT_E_NOMEM && rc != GFT_E_UNSUPPORTED) return rc;
            err.clear();
        }
        if (r && (rc = json_staged(e, *r, d_blob, d_doc_off, n_docs, d_status, d_rows, want_tags, staged, err))) return rc;
    }
    if (!r) return by_host();
    return json_results(*r, blob, doc_off, n_docs, staged, want_tags, out, err);
}

int GroupFinder::ProcessJsonsSchema(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, std::vector<DocResult>& out, Error& err,
                                    ResultText* text) {
    return jsons_schema(blob, doc_off, n_docs, false, out, err, text);
}

int GroupFinder::jsons_schema(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, bool want_tags, std::vector<DocResult>& out, Error& err,
                              ResultText* text, JsonLines* lines) {
    Records* r = schema_records("JSON batch", err);
    if (!r) return GFT_E_INVALID;
    int rc = json_ready(nullptr, *r, err);
    if (rc) return rc;
    if ((rc = compile(*r, err))) return rc;
    if (!lines && (rc = json_check_offsets(doc_off, n_docs, err))) return rc;
    // (the schema's own lists; it is compiled already, whatever the batch holds)
    return json_batch(blob, doc_off, n_docs, r->inc, r->exc, want_tags, r->row_words(),
                      [&](gft_engine*, const uint8_t*, const uint64_t*, uint64_t, int&) { return rec_; }, out, err, text, lines);
}

// ---- the schema discovered from the batch ------------------------------------------------------------------------------------
int GroupFinder::JsonPathsDevice(const uint8_t* d_blob, const uint64_t* d_doc_off, uint64_t n_docs, std::vector<std::string>& paths,
                                 uint64_t* dropped, Error& err) {
    gft_engine* e = nullptr;
    int rc = single_device_engine(findthem_, "JSON batches", e, err);
    if (rc) return rc;
    RulesLock whole_call(e);               // (the set and the pool are the engine's)
    rc = json_paths_device(e, d_blob, d_doc_off, n_docs, paths, dropped);
    if (rc) err = gft_last_error(e);
    return rc;
}

int GroupFinder::ProcessJsonsAuto(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const std::vector<std::string>& includePaths,
                                  const std::vector<std::string>& excludePaths, std::vector<DocResult>& out, Error& err, ResultText* text) {
    return jsons_auto(blob, doc_off, n_docs, includePaths, excludePaths, false, out, err, text);
}

int GroupFinder::jsons_auto(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const std::vector<std::string>& includePaths,
                            const std::vector<std::string>& excludePaths, bool want_tags, std::vector<DocResult>& out, Error& err,
                            ResultText* text, JsonLines* lines) {
    int rc = lines ? (int)GFT_OK : json_check_offsets(doc_off, n_docs, err);
    if (rc) return rc;
    auto_last_paths = auto_last_dropped = auto_last_recompiled = 0;
    const uint64_t RW = (RuleExprs().size() + 31) / 32;      // (a bit per rule expression, whatever the schema)
    // auto_ for the staged batch, or null: a limit of the schema's compilers, the host route for every document
    auto discover = [&](gft_engine* e, const uint8_t* d_blob, const uint64_t* d_doc_off, uint64_t n_docs, int& rc) -> std::shared_ptr<Records> {
        std::vector<std::string> found;
        if ((rc = json_paths_device(e, d_blob, d_doc_off, n_docs, found, &auto_last_dropped))) { err = gft_last_error(e); return nullptr; }
        auto_last_paths = found.size();
        // the kept schema answers when it covers the batch and was made for these lists
        const bool same_lists = auto_ && auto_->inc == includePaths && auto_->exc == excludePaths;
        bool covered = same_lists;
        if (covered) {
            const std::set<std::string> kept(auto_->schema.begin(), auto_->schema.end());
            for (const auto& p : found) covered = covered && kept.count(p);
        }
        if (!covered) {
            // what was kept stays in when the whole still compiles, so that batches of alternating shapes settle
            std::vector<std::vector<std::string>> tries;
            if (same_lists) {
                std::set<std::string> all(auto_->schema.begin(), auto_->schema.end());
                all.insert(found.begin(), found.end());
                if (all.size() <= kJsonPathCap) tries.emplace_back(all.begin(), all.end());
            }
            tries.push_back(found);
            std::shared_ptr<Records> next;
            for (const auto& paths : tries) {
                auto r = std::make_shared<Records>();
                Error why;
                rc = make_records(paths, includePaths, excludePaths, *r, why);
                if (!rc) rc = r->json_rc;                      // (here a schema without a trie is no schema)
                if (rc == GFT_E_UNSUPPORTED) continue;         // a limit: never the caller's error
                if (rc) { err = why.empty() ? r->json_err : why; return nullptr; }
                next = std::move(r);
                break;
            }
            rc = GFT_OK;
            auto_last_recompiled = 1;
            if (!next) return nullptr;
            auto_ = std::move(next);
        } else if (auto_->rules_version != rules_version_ || auto_->n_exprs != findthem_->expressions().size()) {
            auto_last_recompiled = 1;      // (compile, below)
        }
        rc = compile(*auto_, err);                             // (rules or expressions were added since)
        if (rc == GFT_E_UNSUPPORTED) { err.clear(); rc = GFT_OK; auto_.reset(); return nullptr; }   // (its rules no longer compile)
        if (rc) return nullptr;
        if (!want_tags && auto_->row_words() != RW) { err = "ProcessJsonsAuto: the rule set's rows are not those the batch was staged for"; rc = GFT_E_INTERNAL; return nullptr; }
        return auto_;
    };
    return json_batch(blob, doc_off, n_docs, includePaths, excludePaths, want_tags, RW, discover, out, err, text, lines);
}

// ---- JSON Lines: the batch arrives as one blob, a document a line ----------------------------------------------------------------
int GroupFinder::ProcessJsonLines(const uint8_t* blob, uint64_t len, const std::vector<std::string>& includePaths,
                                  const std::vector<std::string>& excludePaths, std::vector<DocResult>& out, Error& err, ResultText* text) {
    JsonLines lines;
    lines.len = len;
    if (!rec_) return jsons_auto(blob, nullptr, 0, includePaths, excludePaths, false, out, err, text, &lines);
    if (!includePaths.empty() || !excludePaths.empty()) {
        err = "ProcessJsonLines: a schema is set, its include and exclude lists answer (pass none)";
        return GFT_E_INVALID;
    }
    return jsons_schema(blob, nullptr, 0, false, out, err, text, &lines);
}

int64_t GroupFinder::DebugJsonFind(int64_t parent, const uint8_t* key, uint32_t key_len, int64_t* field) {
    if (field) *field = -1;
    if (!rec_ || rec_->json_rc || parent < 0 || parent >= (int64_t)rec_->json.nodes.size() || (key_len && !key)) return -1;
    const uint32_t c = key_len ? json_schema_find(rec_->json, (uint32_t)parent, key, key_len) : (uint32_t)parent;
    if (c == kJsonNone) return -1;
    if (field && rec_->json.nodes[c].field != kJsonNone) *field = rec_->json.nodes[c].field;
    return c;
}

int GroupFinder::DebugJsonLeaves(bool emulate, const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, uint8_t* status, uint64_t* rec_off,
                                 uint32_t* leaf_field, uint64_t* leaf_off, uint64_t leaf_cap, uint8_t* text, uint64_t text_cap, uint64_t* totals,
                                 Error& err) {
    Records* r = schema_records("JSON batch", err);
    if (!r) return GFT_E_INVALID;
    int rc = json_ready(nullptr, *r, err);
    if (rc) return rc;
    const JsonLeavesOut out{status, rec_off, leaf_field, leaf_off, leaf_cap, text, text_cap, totals};
    return emulate ? json_leaves_emulate(r->json, blob, doc_off, n_docs, out, err) : json_leaves_ref(r->schema, blob, doc_off, n_docs, out, err);
}

}  // namespace gft
