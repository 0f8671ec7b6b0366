// group_api.cpp -- the group finder behind the C ABI (include/gft.h: gft_group_*, and the gft_debug_* calls that take a group):
// the handle, argument decoding, and the JSON documents that go out.  What the calls do is GroupFinder's (group_host.hpp).
#include <algorithm>
#include <cstring>
#include <mutex>

#include "gft_guard.hpp"
#include "group_host.hpp"
#include "host_parallel.hpp"
#include "json_paths.hpp"
#include "rules_json.hpp"
#include "tags_json.hpp"

using namespace gft;

struct gft_group {
    std::unique_ptr<GroupFinder> g;
    std::string err;
    std::string result;      // the last gft_group_process_jsons document (gft_group_last_result)
    mutable std::recursive_mutex mu;   // one caller at a time per handle
};
#define GFT_GLOCK(g) std::lock_guard<std::recursive_mutex> _gft_glock((g)->mu)

// finder_host.cpp
Finder* gft_finder_impl(gft_finder* f);

namespace {

int put(const std::string& s, char* out, uint64_t cap, uint64_t* needed) {
    if (needed) *needed = s.size() + 1;
    if (!out || cap < s.size() + 1) return GFT_E_INVALID;
    memcpy(out, s.c_str(), s.size() + 1);
    return GFT_OK;
}

// sorted paths -> blob + offsets under the cap / needed convention: needed[0] bytes, needed[1] paths; path_off [path_cap + 1]
int put_paths(const std::vector<std::string>& paths, uint8_t* blob, uint64_t blob_cap, uint64_t* path_off, uint64_t path_cap, uint64_t* needed,
              uint64_t* n_paths) {
    uint64_t bytes = 0;
    for (const auto& p : paths) bytes += p.size();
    if (needed) { needed[0] = bytes; needed[1] = paths.size(); }
    if (n_paths) *n_paths = paths.size();
    if (bytes > blob_cap || paths.size() > path_cap || !path_off || (bytes && !blob)) return GFT_E_INVALID;
    uint64_t at = 0;
    for (size_t i = 0; i < paths.size(); i++) {
        path_off[i] = at;
        if (!paths[i].empty()) memcpy(blob + at, paths[i].data(), paths[i].size());
        at += paths[i].size();
    }
    path_off[paths.size()] = at;
    return GFT_OK;
}

void str_array(const std::vector<std::string>& v, std::string& o) {
    o += "[";
    for (size_t i = 0; i < v.size(); i++) { if (i) o += ","; dsl::json_str(v[i], o); }
    o += "]";
}

void rules_json(const GroupFinder::RuleResult& r, std::string& o) {
    o += "{";
    bool first = true;
    for (const auto& kv : r) {
        if (!first) o += ",";
        first = false;
        dsl::json_str(kv.first, o);
        o += ":";
        str_array(kv.second, o);
    }
    o += "}";
}

bool string_list(const uint8_t* p, uint64_t n, std::vector<std::string>& out, std::string& err) {
    out.clear();
    if (!p || !n) return true;
    json::Value v;
    err = json::Parse((const char*)p, n, v);
    if (!err.empty()) return false;
    if (v.kind == json::Value::Null) return true;
    if (v.kind != json::Value::Array) { err = "expected a JSON array of strings"; return false; }
    for (const auto& x : v.arr) {
        if (x.kind != json::Value::String) { err = "expected a JSON array of strings"; return false; }
        out.push_back(x.str);
    }
    return true;
}

// the result document of a JSON batch into g->result (what: 0 rules, 1 tags)
void result_document(gft_group* g, const std::vector<GroupFinder::DocResult>& res, int what) {
    std::vector<std::string> parts(res.size());
    parallel_for(res.size(), [&](uint64_t d, unsigned) {
        std::string& o = parts[d];
        if (what == 0) { rule_doc_text(res[d].err, res[d].rules, o); return; }     // (the text a hole of the device route gets, too)
        tag_doc_text(res[d].err, res[d].tags, o);
    });
    size_t total = 2;
    for (const auto& p : parts) total += p.size() + 1;
    std::string& o = g->result;
    o.clear();
    o.reserve(total);
    o = "[";
    for (size_t d = 0; d < parts.size(); d++) { if (d) o += ","; o += parts[d]; }
    o += "]";
}

bool tagmap_from_json(const json::Value& v, gdsl::TagMap& m, std::string& err) {
    if (v.kind != json::Value::Object) { err = "expected {tag: {field: [expressions]}}"; return false; }
    for (const auto& t : v.obj) {
        auto& fields = m[t.first];
        if (t.second.kind == json::Value::Null) continue;
        if (t.second.kind != json::Value::Object) { err = "expected {tag: {field: [expressions]}}"; return false; }
        for (const auto& fp : t.second.obj) {
            auto& set = fields[fp.first];
            if (fp.second.kind == json::Value::Array)
                for (const auto& x : fp.second.arr) if (x.kind == json::Value::String) set.insert(x.str);
        }
    }
    return true;
}

}  // namespace

extern "C" {

int gft_group_create(gft_group** out, gft_finder* finder) try {
    if (!out || !finder) return GFT_E_INVALID;
    gft_group* g = new gft_group();
    g->g.reset(new GroupFinder(gft_finder_impl(finder)));
    *out = g;
    return GFT_OK;
} GFT_CATCH(nullptr)
void gft_group_destroy(gft_group* g) { delete g; }
const char* gft_group_last_error(const gft_group* g) { return g ? g->err.c_str() : "null group finder"; }

int gft_group_add_rule(gft_group* g, const uint8_t* name, uint64_t name_len, const uint8_t* expr, uint64_t expr_len) try {
    if (!g) return GFT_E_INVALID;
    GFT_GLOCK(g);
    g->err = g->g->AddRule(std::string((const char*)name, name_len), {std::string((const char*)expr, expr_len)});
    return g->err.empty() ? GFT_OK : GFT_E_PARSE;
} GFT_CATCH((g ? &const_cast<gft_group*>(g)->err : nullptr))

int gft_group_state(const gft_group* g, char* out, uint64_t cap, uint64_t* needed) try {
    if (!g) return GFT_E_INVALID;
    GFT_GLOCK(g);
    std::string o = "{\"rules\":{";
    bool first = true;
    for (const auto& kv : g->g->rules()) {
        if (!first) o += ",";
        first = false;
        dsl::json_str(kv.first, o);
        o += ":[";
        for (size_t i = 0; i < kv.second.size(); i++) {
            if (i) o += ",";
            o += "{\"ExpressionString\":";
            dsl::json_str(kv.second[i].ExpressionString, o);
            o += ",\"Expression\":" + gdsl::ToJson(*kv.second[i].Expression) + "}";
        }
        o += "]";
    }
    o += "},\"fields\":";
    str_array({g->g->fields().begin(), g->g->fields().end()}, o);
    o += ",\"tags\":";
    str_array({g->g->tags().begin(), g->g->tags().end()}, o);
    o += "}";
    return put(o, out, cap, needed);
} GFT_CATCH((g ? &const_cast<gft_group*>(g)->err : nullptr))

int gft_group_process_jsons(gft_group* g, const uint8_t* json_blob, const uint64_t* doc_off, uint64_t n_docs,
                            const uint8_t* include_json, uint64_t include_len, const uint8_t* exclude_json,
                            uint64_t exclude_len, int what, char* out, uint64_t cap, uint64_t* needed) try {
    if (!g || (n_docs && (!json_blob || !doc_off))) return GFT_E_INVALID;
    GFT_GLOCK(g);
    std::vector<std::string> inc, exc;
    if (!string_list(include_json, include_len, inc, g->err) || !string_list(exclude_json, exclude_len, exc, g->err))
        return GFT_E_INVALID;
    std::vector<GroupFinder::DocResult> res;
    g->err = g->g->ProcessJsons(json_blob, doc_off, n_docs, inc, exc, what != 0, res);
    if (!g->err.empty()) return GFT_E_ENGINE;
    result_document(g, res, what);
    return put(g->result, out, cap, needed);
} GFT_CATCH((g ? &const_cast<gft_group*>(g)->err : nullptr))

int gft_group_process_jsons_schema(gft_group* g, const uint8_t* json_blob, const uint64_t* doc_off, uint64_t n_docs, char* out, uint64_t cap,
                                   uint64_t* needed) try {
    if (!g || !doc_off || (n_docs && !json_blob)) return GFT_E_INVALID;
    GFT_GLOCK(g);
    std::vector<GroupFinder::DocResult> res;
    GroupFinder::ResultText text{&g->result, false};
    int rc = g->g->ProcessJsonsSchema(json_blob, doc_off, n_docs, res, g->err, &text);
    if (rc) return rc;
    if (!text.written) result_document(g, res, 0);
    return put(g->result, out, cap, needed);
} GFT_CATCH((g ? &g->err : nullptr))

int gft_group_json_last(const gft_group* g, uint64_t* n_device, uint64_t* n_host) try {
    if (!g) return GFT_E_INVALID;
    GFT_GLOCK(g);
    if (n_device) *n_device = g->g->json_last_device;
    if (n_host) *n_host = g->g->json_last_host;
    return GFT_OK;
} GFT_CATCH((g ? &const_cast<gft_group*>(g)->err : nullptr))

int gft_group_json_paths_device(gft_group* g, const uint8_t* d_json_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint8_t* paths_blob,
                                uint64_t blob_cap, uint64_t* path_off, uint64_t path_cap, uint64_t* needed, uint64_t* n_paths, uint64_t* dropped) try {
    if (!g) return GFT_E_INVALID;
    GFT_GLOCK(g);
    std::vector<std::string> paths;
    int rc = g->g->JsonPathsDevice(d_json_blob, d_doc_off, n_docs, paths, dropped, g->err);
    if (rc) return rc;
    if ((rc = put_paths(paths, paths_blob, blob_cap, path_off, path_cap, needed, n_paths))) g->err = "gft_group_json_paths_device: the paths do not fit the caps";
    return rc;
} GFT_CATCH((g ? &g->err : nullptr))

int gft_group_process_jsons_auto(gft_group* g, const uint8_t* json_blob, const uint64_t* doc_off, uint64_t n_docs, const uint8_t* include_json,
                                 uint64_t include_len, const uint8_t* exclude_json, uint64_t exclude_len, char* out, uint64_t cap,
                                 uint64_t* needed) try {
    if (!g || !doc_off || (n_docs && !json_blob)) return GFT_E_INVALID;
    GFT_GLOCK(g);
    std::vector<std::string> inc, exc;
    if (!string_list(include_json, include_len, inc, g->err) || !string_list(exclude_json, exclude_len, exc, g->err)) return GFT_E_INVALID;
    std::vector<GroupFinder::DocResult> res;
    GroupFinder::ResultText text{&g->result, false};
    int rc = g->g->ProcessJsonsAuto(json_blob, doc_off, n_docs, inc, exc, res, g->err, &text);
    if (rc) return rc;
    if (!text.written) result_document(g, res, 0);
    return put(g->result, out, cap, needed);
} GFT_CATCH((g ? &g->err : nullptr))

int gft_group_process_json_lines(gft_group* g, const uint8_t* blob, uint64_t len, const uint8_t* include_json, uint64_t include_len,
                                 const uint8_t* exclude_json, uint64_t exclude_len, char* out, uint64_t cap, uint64_t* needed) try {
    if (!g || (len && !blob)) return GFT_E_INVALID;
    GFT_GLOCK(g);
    std::vector<std::string> inc, exc;
    if (!string_list(include_json, include_len, inc, g->err) || !string_list(exclude_json, exclude_len, exc, g->err)) return GFT_E_INVALID;
    std::vector<GroupFinder::DocResult> res;
    GroupFinder::ResultText text{&g->result, false};
    int rc = g->g->ProcessJsonLines(blob, len, inc, exc, res, g->err, &text);
    if (rc) return rc;
    if (!text.written) result_document(g, res, 0);
    return put(g->result, out, cap, needed);
} GFT_CATCH((g ? &g->err : nullptr))

int gft_group_json_auto_last(const gft_group* g, uint64_t* n_paths, uint64_t* dropped, uint64_t* recompiled) try {
    if (!g) return GFT_E_INVALID;
    GFT_GLOCK(g);
    if (n_paths) *n_paths = g->g->auto_last_paths;
    if (dropped) *dropped = g->g->auto_last_dropped;
    if (recompiled) *recompiled = g->g->auto_last_recompiled;
    return GFT_OK;
} GFT_CATCH((g ? &const_cast<gft_group*>(g)->err : nullptr))

int gft_debug_emulate_json_paths(gft_group* g, const uint8_t* json_blob, const uint64_t* doc_off, uint64_t n_docs, uint8_t* paths_blob,
                                 uint64_t blob_cap, uint64_t* path_off, uint64_t path_cap, uint64_t* needed, uint64_t* n_paths, uint64_t* dropped,
                                 uint64_t* hashes, uint64_t hash_cap, uint64_t* n_hashes) try {
    if (!g || (n_docs && !doc_off)) return GFT_E_INVALID;
    GFT_GLOCK(g);
    std::vector<std::string> paths;
    std::vector<uint64_t> set;
    int rc = json_paths_emulate(json_blob, doc_off, n_docs, paths, &set, dropped, g->err);
    if (rc) return rc;
    if (n_hashes) *n_hashes = set.size();
    if (hashes) memcpy(hashes, set.data(), (size_t)std::min<uint64_t>(hash_cap, set.size()) * 8);
    if ((rc = put_paths(paths, paths_blob, blob_cap, path_off, path_cap, needed, n_paths))) g->err = "gft_debug_emulate_json_paths: the paths do not fit the caps";
    return rc;
} GFT_CATCH((g ? &g->err : nullptr))

int gft_debug_json_paths_ref(gft_group* g, const uint8_t* json_blob, const uint64_t* doc_off, uint64_t n_docs, uint8_t* paths_blob, uint64_t blob_cap,
                             uint64_t* path_off, uint64_t path_cap, uint64_t* needed, uint64_t* n_paths) try {
    if (!g || (n_docs && !doc_off)) return GFT_E_INVALID;
    GFT_GLOCK(g);
    std::vector<std::string> paths;
    int rc = json_paths_ref(json_blob, doc_off, n_docs, paths, g->err);
    if (rc) return rc;
    if ((rc = put_paths(paths, paths_blob, blob_cap, path_off, path_cap, needed, n_paths))) g->err = "gft_debug_json_paths_ref: the paths do not fit the caps";
    return rc;
} GFT_CATCH((g ? &g->err : nullptr))

int gft_group_json_leaves_device(gft_group* g, const uint8_t* d_json_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint8_t* d_status,
                                 uint64_t* d_rec_off, uint32_t* d_leaf_field, uint64_t* d_leaf_off, uint64_t leaf_cap, uint8_t* d_text,
                                 uint64_t text_cap, uint64_t* totals) try {
    if (!g) return GFT_E_INVALID;
    GFT_GLOCK(g);
    return g->g->JsonLeavesDevice(d_json_blob, d_doc_off, n_docs, d_status, d_rec_off, d_leaf_field, d_leaf_off, leaf_cap, d_text, text_cap, totals,
                                  g->err);
} GFT_CATCH((g ? &g->err : nullptr))

int gft_group_process_jsons_device(gft_group* g, const uint8_t* d_json_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint8_t* d_status,
                                   uint32_t* d_rule_bitmap) try {
    if (!g) return GFT_E_INVALID;
    GFT_GLOCK(g);
    return g->g->ProcessJsonsDevice(d_json_blob, d_doc_off, n_docs, d_status, d_rule_bitmap, g->err);
} GFT_CATCH((g ? &g->err : nullptr))

int gft_debug_json_leaves_ref(gft_group* g, const uint8_t* json_blob, const uint64_t* doc_off, uint64_t n_docs, uint8_t* status, uint64_t* rec_off,
                              uint32_t* leaf_field, uint64_t* leaf_off, uint64_t leaf_cap, uint8_t* text, uint64_t text_cap, uint64_t* totals) try {
    if (!g) return GFT_E_INVALID;
    GFT_GLOCK(g);
    return g->g->DebugJsonLeaves(false, json_blob, doc_off, n_docs, status, rec_off, leaf_field, leaf_off, leaf_cap, text, text_cap, totals, g->err);
} GFT_CATCH((g ? &g->err : nullptr))

int gft_debug_emulate_json_leaves(gft_group* g, const uint8_t* json_blob, const uint64_t* doc_off, uint64_t n_docs, uint8_t* status,
                                  uint64_t* rec_off, uint32_t* leaf_field, uint64_t* leaf_off, uint64_t leaf_cap, uint8_t* text, uint64_t text_cap,
                                  uint64_t* totals) try {
    if (!g) return GFT_E_INVALID;
    GFT_GLOCK(g);
    return g->g->DebugJsonLeaves(true, json_blob, doc_off, n_docs, status, rec_off, leaf_field, leaf_off, leaf_cap, text, text_cap, totals, g->err);
} GFT_CATCH((g ? &g->err : nullptr))

int64_t gft_debug_json_schema_find(gft_group* g, int64_t parent, const uint8_t* key, uint32_t key_len, int64_t* field) try {
    if (!g) return -2;
    GFT_GLOCK(g);
    return g->g->DebugJsonFind(parent, key, key_len, field);
} GFT_CATCH_VALUE(-2)

int gft_group_last_result(const gft_group* g, char* out, uint64_t cap, uint64_t* needed) try {
    if (!g) return GFT_E_INVALID;
    GFT_GLOCK(g);
    return put(g->result, out, cap, needed);
} GFT_CATCH((g ? &const_cast<gft_group*>(g)->err : nullptr))

int gft_group_evaluate(gft_group* g, const uint8_t* tagmap, uint64_t len, char* out, uint64_t cap, uint64_t* needed) try {
    if (!g || !tagmap) return GFT_E_INVALID;
    GFT_GLOCK(g);
    json::Value v;
    g->err = json::Parse((const char*)tagmap, len, v);
    gdsl::TagMap m;
    if (!g->err.empty() || !tagmap_from_json(v, m, g->err)) return GFT_E_INVALID;
    GroupFinder::RuleResult rr;
    g->err = g->g->EvaluateRules(m, rr);
    if (!g->err.empty()) return GFT_E_ENGINE;
    std::string o;
    rules_json(rr, o);
    return put(o, out, cap, needed);
} GFT_CATCH((g ? &const_cast<gft_group*>(g)->err : nullptr))

int gft_group_set_schema(gft_group* g, const uint8_t* paths_blob, const uint64_t* path_off, uint32_t n_fields, const uint8_t* include_json,
                         uint64_t include_len, const uint8_t* exclude_json, uint64_t exclude_len) try {
    if (!g || (n_fields && !path_off)) return GFT_E_INVALID;
    GFT_GLOCK(g);
    std::vector<std::string> inc, exc, paths;
    if (!string_list(include_json, include_len, inc, g->err) || !string_list(exclude_json, exclude_len, exc, g->err)) return GFT_E_INVALID;
    for (uint32_t f = 0; f < n_fields; f++) {
        if (path_off[f] > path_off[f + 1] || (path_off[f + 1] > path_off[f] && !paths_blob)) { g->err = "record schema: broken path offsets"; return GFT_E_INVALID; }
        paths.emplace_back(paths_blob ? (const char*)paths_blob + path_off[f] : "", (size_t)(path_off[f + 1] - path_off[f]));
    }
    return g->g->SetSchema(paths, inc, exc, g->err);
} GFT_CATCH((g ? &g->err : nullptr))

uint32_t gft_group_n_rule_exprs(gft_group* g) try {
    if (!g) return 0;
    GFT_GLOCK(g);
    return (uint32_t)g->g->RuleExprs().size();
} GFT_CATCH_VALUE(0)

int gft_group_rule_expr(gft_group* g, uint32_t i, const uint8_t** name, uint32_t* name_len, const uint8_t** expr, uint32_t* expr_len) try {
    if (!g) return GFT_E_INVALID;
    GFT_GLOCK(g);
    const auto& v = g->g->RuleExprs();
    if (i >= v.size()) { g->err = "gft_group_rule_expr: index out of range"; return GFT_E_INVALID; }
    if (name) *name = (const uint8_t*)v[i].name->data();
    if (name_len) *name_len = (uint32_t)v[i].name->size();
    if (expr) *expr = (const uint8_t*)v[i].expr->data();
    if (expr_len) *expr_len = (uint32_t)v[i].expr->size();
    return GFT_OK;
} GFT_CATCH((g ? &g->err : nullptr))

int gft_group_process_records_device(gft_group* g, const uint8_t* d_text_blob, const uint64_t* d_leaf_off, const uint32_t* d_leaf_field,
                                     const uint64_t* d_rec_off, uint64_t n_records, uint64_t n_leaves, uint32_t* d_rule_bitmap) try {
    if (!g) return GFT_E_INVALID;
    GFT_GLOCK(g);
    return g->g->ProcessRecordsDevice(d_text_blob, d_leaf_off, d_leaf_field, d_rec_off, n_records, n_leaves, d_rule_bitmap, g->err);
} GFT_CATCH((g ? &g->err : nullptr))

int gft_group_process_records(gft_group* g, const uint8_t* text_blob, const uint64_t* leaf_off, const uint32_t* leaf_field,
                              const uint64_t* rec_off, uint64_t n_records, uint64_t n_leaves, uint32_t* rule_bitmap) try {
    if (!g) return GFT_E_INVALID;
    GFT_GLOCK(g);
    return g->g->ProcessRecords(text_blob, leaf_off, leaf_field, rec_off, n_records, n_leaves, rule_bitmap, g->err);
} GFT_CATCH((g ? &g->err : nullptr))

int gft_debug_eval_rules(gft_group* g, const uint32_t* hit_bitmap, uint32_t n_exprs, const uint32_t* leaf_field, const uint64_t* rec_off,
                         uint64_t n_records, uint64_t n_leaves, uint32_t* rule_bitmap) try {
    if (!g) return GFT_E_INVALID;
    GFT_GLOCK(g);
    return g->g->DebugEvalRules(hit_bitmap, n_exprs, leaf_field, rec_off, n_records, n_leaves, rule_bitmap, g->err);
} GFT_CATCH((g ? &g->err : nullptr))

int gft_debug_eval_rules_device(gft_group* g, const uint32_t* d_hit_bitmap, uint32_t n_exprs, const uint32_t* d_leaf_field,
                                const uint64_t* d_rec_off, uint64_t n_records, uint64_t n_leaves, uint32_t* d_rule_bitmap) try {
    if (!g) return GFT_E_INVALID;
    GFT_GLOCK(g);
    return g->g->DebugEvalRulesDevice(d_hit_bitmap, n_exprs, d_leaf_field, d_rec_off, n_records, n_leaves, d_rule_bitmap, g->err);
} GFT_CATCH((g ? &g->err : nullptr))

int gft_group_tag_records_device(gft_group* g, const uint8_t* d_text_blob, const uint64_t* d_leaf_off, const uint32_t* d_leaf_field,
                                 const uint64_t* d_rec_off, uint64_t n_records, uint64_t n_leaves, uint64_t* d_row_off, uint32_t* d_ent_field,
                                 uint32_t* d_ent_expr, uint32_t* d_ent_tag, uint64_t cap, uint64_t* total) try {
    if (!g) return GFT_E_INVALID;
    GFT_GLOCK(g);
    return g->g->TagRecordsDevice(d_text_blob, d_leaf_off, d_leaf_field, d_rec_off, n_records, n_leaves,
                                  {d_row_off, d_ent_field, d_ent_expr, d_ent_tag, cap, total}, g->err);
} GFT_CATCH((g ? &g->err : nullptr))

int gft_group_tag_records(gft_group* g, const uint8_t* text_blob, const uint64_t* leaf_off, const uint32_t* leaf_field, const uint64_t* rec_off,
                          uint64_t n_records, uint64_t n_leaves, uint64_t* row_off, uint32_t* ent_field, uint32_t* ent_expr, uint32_t* ent_tag,
                          uint64_t cap, uint64_t* total) try {
    if (!g) return GFT_E_INVALID;
    GFT_GLOCK(g);
    return g->g->TagRecords(text_blob, leaf_off, leaf_field, rec_off, n_records, n_leaves, {row_off, ent_field, ent_expr, ent_tag, cap, total}, g->err);
} GFT_CATCH((g ? &g->err : nullptr))

int gft_group_tag_jsons_device(gft_group* g, const uint8_t* d_json_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint8_t* d_status,
                               uint64_t* d_row_off, uint32_t* d_ent_field, uint32_t* d_ent_expr, uint32_t* d_ent_tag, uint64_t cap,
                               uint64_t* total) try {
    if (!g) return GFT_E_INVALID;
    GFT_GLOCK(g);
    return g->g->TagJsonsDevice(d_json_blob, d_doc_off, n_docs, d_status, {d_row_off, d_ent_field, d_ent_expr, d_ent_tag, cap, total}, g->err);
} GFT_CATCH((g ? &g->err : nullptr))

int gft_group_tag_jsons_schema(gft_group* g, const uint8_t* json_blob, const uint64_t* doc_off, uint64_t n_docs, char* out, uint64_t cap,
                               uint64_t* needed) try {
    if (!g || !doc_off || (n_docs && !json_blob)) return GFT_E_INVALID;
    GFT_GLOCK(g);
    std::vector<GroupFinder::DocResult> res;
    GroupFinder::ResultText text{&g->result, false};
    int rc = g->g->TagJsonsSchema(json_blob, doc_off, n_docs, res, g->err, &text);
    if (rc) return rc;
    if (!text.written) result_document(g, res, 1);
    return put(g->result, out, cap, needed);
} GFT_CATCH((g ? &g->err : nullptr))

int gft_group_tag_jsons_auto(gft_group* g, const uint8_t* json_blob, const uint64_t* doc_off, uint64_t n_docs, const uint8_t* include_json,
                             uint64_t include_len, const uint8_t* exclude_json, uint64_t exclude_len, char* out, uint64_t cap,
                             uint64_t* needed) try {
    if (!g || !doc_off || (n_docs && !json_blob)) return GFT_E_INVALID;
    GFT_GLOCK(g);
    std::vector<std::string> inc, exc;
    if (!string_list(include_json, include_len, inc, g->err) || !string_list(exclude_json, exclude_len, exc, g->err)) return GFT_E_INVALID;
    std::vector<GroupFinder::DocResult> res;
    GroupFinder::ResultText text{&g->result, false};
    int rc = g->g->TagJsonsAuto(json_blob, doc_off, n_docs, inc, exc, res, g->err, &text);
    if (rc) return rc;
    if (!text.written) result_document(g, res, 1);
    return put(g->result, out, cap, needed);
} GFT_CATCH((g ? &g->err : nullptr))

int gft_debug_tag_entries(gft_group* g, const uint32_t* hit_bitmap, uint32_t n_exprs, const uint32_t* leaf_field, const uint64_t* rec_off,
                          uint64_t n_records, uint64_t n_leaves, uint64_t* row_off, uint32_t* ent_field, uint32_t* ent_expr, uint32_t* ent_tag,
                          uint64_t cap, uint64_t* total) try {
    if (!g) return GFT_E_INVALID;
    GFT_GLOCK(g);
    return g->g->DebugTagEntries(hit_bitmap, n_exprs, leaf_field, rec_off, n_records, n_leaves, {row_off, ent_field, ent_expr, ent_tag, cap, total},
                                 g->err);
} GFT_CATCH((g ? &g->err : nullptr))

int gft_debug_tag_entries_device(gft_group* g, const uint32_t* d_hit_bitmap, uint32_t n_exprs, const uint32_t* d_leaf_field,
                                 const uint64_t* d_rec_off, uint64_t n_records, uint64_t n_leaves, uint64_t* d_row_off, uint32_t* d_ent_field,
                                 uint32_t* d_ent_expr, uint32_t* d_ent_tag, uint64_t cap, uint64_t* total) try {
    if (!g) return GFT_E_INVALID;
    GFT_GLOCK(g);
    return g->g->DebugTagEntriesDevice(d_hit_bitmap, n_exprs, d_leaf_field, d_rec_off, n_records, n_leaves,
                                       {d_row_off, d_ent_field, d_ent_expr, d_ent_tag, cap, total}, g->err);
} GFT_CATCH((g ? &g->err : nullptr))

int gft_group_rules_json_device(gft_group* g, const uint32_t* d_rule_bitmap, uint64_t n_docs, const uint64_t* d_hole_len, uint8_t* d_out, uint64_t cap,
                                uint64_t* d_out_off, uint64_t* total) try {
    if (!g) return GFT_E_INVALID;
    GFT_GLOCK(g);
    return g->g->RulesJsonDevice(d_rule_bitmap, n_docs, d_hole_len, d_out, cap, d_out_off, total, g->err);
} GFT_CATCH((g ? &g->err : nullptr))

int gft_debug_rules_json(gft_group* g, const uint32_t* rule_bitmap, uint64_t n_docs, const uint64_t* hole_len, uint8_t* out, uint64_t cap,
                         uint64_t* out_off, uint64_t* total) try {
    if (!g) return GFT_E_INVALID;
    GFT_GLOCK(g);
    return g->g->DebugRulesJson(rule_bitmap, n_docs, hole_len, out, cap, out_off, total, g->err);
} GFT_CATCH((g ? &g->err : nullptr))

int gft_group_tags_json_device(gft_group* g, const uint32_t* d_hit_bitmap, const uint32_t* d_leaf_field, const uint64_t* d_rec_off, uint64_t n_records,
                               uint64_t n_leaves, const uint64_t* d_hole_len, uint8_t* d_out, uint64_t cap, uint64_t* d_out_off, uint64_t* total) try {
    if (!g) return GFT_E_INVALID;
    GFT_GLOCK(g);
    return g->g->TagsJsonDevice(d_hit_bitmap, d_leaf_field, d_rec_off, n_records, n_leaves, d_hole_len, d_out, cap, d_out_off, total, g->err);
} GFT_CATCH((g ? &g->err : nullptr))

int gft_debug_tags_json(gft_group* g, const uint32_t* hit_bitmap, uint32_t n_exprs, const uint32_t* leaf_field, const uint64_t* rec_off,
                        uint64_t n_records, uint64_t n_leaves, const uint64_t* hole_len, uint8_t* out, uint64_t cap, uint64_t* out_off,
                        uint64_t* total) try {
    if (!g) return GFT_E_INVALID;
    GFT_GLOCK(g);
    return g->g->DebugTagsJson(hit_bitmap, n_exprs, leaf_field, rec_off, n_records, n_leaves, hole_len, out, cap, out_off, total, g->err);
} GFT_CATCH((g ? &g->err : nullptr))

int gft_group_last_batch(const gft_group* g, uint64_t* leaves, uint64_t* bytes) try {
    if (!g) return GFT_E_INVALID;
    GFT_GLOCK(g);
    if (leaves) *leaves = g->g->last_leaves;
    if (bytes) *bytes = g->g->last_bytes;
    return GFT_OK;
} GFT_CATCH((g ? &const_cast<gft_group*>(g)->err : nullptr))

int gft_group_dsl_parse(const uint8_t* expr, uint64_t len, char* out, uint64_t cap, uint64_t* needed) try {
    gdsl::ParseResult pr = gdsl::Parse(std::string((const char*)expr, len));
    std::string o;
    if (!pr.err.empty()) { o = "{\"error\":"; dsl::json_str(pr.err, o); o += "}"; }
    else {
        o = "{\"tree\":" + gdsl::ToJson(*pr.expr) + ",\"tags\":";
        str_array(pr.tags, o);
        o += ",\"fields\":";
        str_array(pr.fields, o);
        o += "}";
    }
    return put(o, out, cap, needed);
} GFT_CATCH(nullptr)

int gft_group_dsl_tokens(const uint8_t* expr, uint64_t len, char* out, uint64_t cap, uint64_t* needed) try {
    const std::string src((const char*)expr, len);
    gdsl::Scanner sc(src);
    std::string o = "[";
    for (int i = 0;; i++) {
        gdsl::ScanResult r = sc.Scan();
        if (i) o += ",";
        o += "{\"Tok\":\"";
        o += gdsl::token_name(r.tok);
        o += "\",\"Lit\":";
        dsl::json_str(r.lit, o);
        o += ",\"Err\":";
        if (r.err.empty()) o += "null"; else dsl::json_str(r.err, o);
        o += "}";
        if (!r.err.empty() || r.tok == gdsl::END_OF_INPUT) break;
    }
    o += "]";
    return put(o, out, cap, needed);
} GFT_CATCH(nullptr)

}  // extern "C"
