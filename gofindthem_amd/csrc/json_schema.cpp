// json_schema.cpp -- the schema trie of the device JSON walker (json_schema.hpp), the walker run on the host, and the
// reference it is tested against.  No device, no handle.
#include "json_schema.hpp"

#include <cstring>
#include <map>
#include <memory>
#include <set>

#include "json_host_wave.hpp"
#include "json_mini.hpp"

namespace gft {

namespace {

std::vector<std::string> split_path(const std::string& p) {
    std::vector<std::string> out;
    if (p.empty()) return out;                        // the root
    size_t a = 0;
    for (;;) {
        const size_t dot = p.find('.', a);
        out.push_back(p.substr(a, dot == std::string::npos ? std::string::npos : dot - a));
        if (dot == std::string::npos) return out;
        a = dot + 1;
    }
}

uint32_t key_hash(const uint8_t* key, uint32_t len) {
    uint32_t h = 0;
    for (uint32_t j = 0; j < len; j++) h += json_key_term(key[j], j);
    return h;
}

}  // namespace

int compile_json_schema(const std::vector<std::string>& paths, JsonSchema& out, std::string& err) {
    JsonSchema s;
    s.n_fields = (uint32_t)paths.size();
    s.nodes.push_back(JsonTrieNode{kJsonNone, 0, 0, kJsonNone});
    std::map<std::pair<uint32_t, std::string>, uint32_t> child;
    for (size_t f = 0; f < paths.size(); f++) {
        uint32_t at = 0;
        for (const std::string& comp : split_path(paths[f])) {
            if (comp.size() > kJsonMaxKey) {
                err = "JSON on the device: a component of schema path " + std::to_string(f) + " is longer than 65535 bytes";
                return GFT_E_UNSUPPORTED;
            }
            auto it = child.find({at, comp});
            if (it == child.end()) {
                if (s.nodes.size() >= kJsonMaxNodes) {
                    err = "JSON on the device: the schema's paths have more than 16384 distinct prefixes (trie nodes)";
                    return GFT_E_UNSUPPORTED;
                }
                const uint32_t id = (uint32_t)s.nodes.size();
                s.nodes.push_back(JsonTrieNode{at, (uint32_t)s.keys.size(), (uint32_t)comp.size(), kJsonNone});
                s.keys.insert(s.keys.end(), comp.begin(), comp.end());
                s.max_key_len = std::max<uint32_t>(s.max_key_len, (uint32_t)comp.size());
                it = child.emplace(std::make_pair(at, comp), id).first;
            }
            at = it->second;
        }
        s.nodes[at].field = (uint32_t)f;               // (gft_group_set_schema refuses a path listed twice)
    }
    s.keys.insert(s.keys.end(), 64, 0);
    size_t size = 16;
    while (size < 2 * s.nodes.size()) size *= 2;
    s.table.assign(size, kJsonNone);
    for (uint32_t id = 1; id < s.nodes.size(); id++) {
        const JsonTrieNode& n = s.nodes[id];
        if (!n.key_len) continue;                      // an empty component: no key reaches it (GFT_JSON_KEY)
        uint32_t slot = json_slot_hash(n.parent, key_hash(s.keys.data() + n.key_off, n.key_len)) & (uint32_t)(size - 1);
        while (s.table[slot] != kJsonNone) slot = (slot + 1) & (uint32_t)(size - 1);
        s.table[slot] = id;
    }
    out = std::move(s);
    return GFT_OK;
}

uint32_t json_schema_find(const JsonSchema& s, uint32_t parent, const uint8_t* key, uint32_t len) {
    if (parent != kJsonNone && parent >= s.nodes.size()) return kJsonNone;
    HostWave w;
    w.m = nullptr;
    return json_trie_find(w, s.view(), parent, JsonKeyMem{key}, len);
}

int json_check_offsets(const uint64_t* doc_off, uint64_t n_docs, std::string& err) {
    for (uint64_t d = 0; d < n_docs; d++) {
        if (doc_off[d] > doc_off[d + 1]) { err = "JSON batch: document offsets descend at document " + std::to_string(d); return GFT_E_INVALID; }
        if (doc_off[d + 1] - doc_off[d] > 0xFFFFFFFFull) { err = "JSON batch: document " + std::to_string(d) + " has 4 GiB or more"; return GFT_E_INVALID; }
    }
    return GFT_OK;
}

namespace {
int check_out(const JsonLeavesOut& o, uint64_t n_docs, std::string& err) {
    if (n_docs && !o.status) { err = "JSON batch: null argument"; return GFT_E_INVALID; }
    if (!o.rec_off) { err = "JSON batch: null argument"; return GFT_E_INVALID; }
    if ((o.leaf_cap && (!o.leaf_field || !o.leaf_off)) || (o.text_cap && !o.text)) { err = "JSON batch: a cap but no array"; return GFT_E_INVALID; }
    return GFT_OK;
}
}  // namespace

int json_leaves_emulate(const JsonSchema& s, const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const JsonLeavesOut& out,
                        std::string& err) {
    int rc = check_out(out, n_docs, err);
    if (rc) return rc;
    if (n_docs && (!blob || !doc_off)) { err = "JSON batch: null argument"; return GFT_E_INVALID; }
    if ((rc = json_check_offsets(doc_off, n_docs, err))) return rc;
    const JsonTrie T = s.view();
    auto mem = std::make_unique<JsonWaveMem>();
    HostWave w;
    w.m = mem.get();
    // json_count
    std::vector<uint32_t> n_leaves(n_docs), n_text(n_docs);
    const JsonDocOut none{nullptr, nullptr, nullptr, 0, 0, 0, 0};
    for (uint64_t d = 0; d < n_docs; d++)
        out.status[d] = (uint8_t)json_walk_doc(w, T, blob + doc_off[d], (uint32_t)(doc_off[d + 1] - doc_off[d]), none, &n_leaves[d], &n_text[d]);
    // json_scan
    std::vector<uint64_t> text_base(n_docs + 1, 0);
    out.rec_off[0] = 0;
    for (uint64_t d = 0; d < n_docs; d++) {
        out.rec_off[d + 1] = out.rec_off[d] + n_leaves[d];
        text_base[d + 1] = text_base[d] + n_text[d];
    }
    if (out.totals) { out.totals[0] = out.rec_off[n_docs]; out.totals[1] = text_base[n_docs]; }
    // json_write
    const bool writes = out.leaf_cap && out.leaf_off;
    for (uint64_t d = 0; d < n_docs; d++) {
        if (out.status[d] || !n_leaves[d]) continue;
        const JsonDocOut O{writes ? out.leaf_field : nullptr, writes ? out.leaf_off : nullptr, out.text_cap ? out.text : nullptr,
                           out.leaf_cap, out.text_cap, out.rec_off[d], text_base[d]};
        uint32_t a, b;
        (void)json_walk_doc(w, T, blob + doc_off[d], (uint32_t)(doc_off[d + 1] - doc_off[d]), O, &a, &b);
    }
    if (out.leaf_off && out.rec_off[n_docs] <= out.leaf_cap) out.leaf_off[out.rec_off[n_docs]] = text_base[n_docs];
    return GFT_OK;
}

// ---- the reference: json_mini's value, walked with paths as lists of components ---------------------------------------
namespace {

struct RefLeaf { uint32_t field; const std::string* text; };

struct RefSchema {
    std::map<std::vector<std::string>, uint32_t> field_of;     // schema paths
    std::set<std::vector<std::string>> prefixes;               // ... and every prefix of one: the trie's nodes
};

// conditions of one document as a set of status bits, its leaves in document order
uint32_t ref_walk(const json::Value& root, const RefSchema& sc, std::vector<RefLeaf>& leaves) {
    uint32_t cond = 0;
    struct Item { const json::Value* v; std::vector<std::string> path; bool known; uint32_t depth; };
    std::vector<Item> todo;
    todo.push_back(Item{&root, {}, true, 0});
    while (!todo.empty()) {
        Item it = std::move(todo.back());
        todo.pop_back();
        const json::Value& v = *it.v;
        if (v.kind == json::Value::String) {
            auto f = it.known ? sc.field_of.find(it.path) : sc.field_of.end();
            if (f == sc.field_of.end()) { cond |= 1u << kJsPath; continue; }
            if (v.str_flags & (json::Value::kRawSurrogate | json::Value::kRawInvalidUtf8)) cond |= 1u << kJsText;
            leaves.push_back(RefLeaf{f->second, &v.str});
        } else if (v.kind == json::Value::Object || v.kind == json::Value::Array) {
            if (it.depth + 1 > kJsonMaxDepth) cond |= 1u << kJsDepth;
            const size_t n = v.kind == json::Value::Object ? v.obj.size() : v.arr.size();
            std::set<std::string> seen;
            std::vector<Item> kids;
            for (size_t i = 0; i < n; i++) {
                Item kid{nullptr, it.path, it.known, it.depth + 1};
                if (v.kind == json::Value::Object) {
                    const std::string& key = v.obj[i].first;
                    kid.v = &v.obj[i].second;
                    const bool bad = key.empty() || (kid.v->key_flags & (json::Value::kRawEscape | json::Value::kRawInvalidUtf8));
                    if (bad) cond |= 1u << kJsKey;
                    kid.path.push_back(key);
                    // a key with '.' names no component; one that is refused names nothing
                    kid.known = it.known && !bad && key.find('.') == std::string::npos && sc.prefixes.count(kid.path);
                    if (kid.known && !seen.insert(key).second) cond |= 1u << kJsDup;
                } else {
                    kid.v = &v.arr[i];
                    kid.path.push_back("index(" + std::to_string(i) + ")");
                    kid.known = it.known && sc.prefixes.count(kid.path);
                }
                kids.push_back(std::move(kid));
            }
            for (size_t i = kids.size(); i-- > 0;) todo.push_back(std::move(kids[i]));     // popped in document order
        }
    }
    return cond;
}

}  // namespace

int json_leaves_ref(const std::vector<std::string>& paths, const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs,
                    const JsonLeavesOut& out, std::string& err) {
    int rc = check_out(out, n_docs, err);
    if (rc) return rc;
    if (n_docs && (!blob || !doc_off)) { err = "JSON batch: null argument"; return GFT_E_INVALID; }
    if ((rc = json_check_offsets(doc_off, n_docs, err))) return rc;
    RefSchema sc;
    for (size_t f = 0; f < paths.size(); f++) {
        std::vector<std::string> comps;
        const std::string& p = paths[f];
        if (!p.empty())
            for (size_t a = 0;;) {
                const size_t dot = p.find('.', a);
                comps.push_back(p.substr(a, dot == std::string::npos ? std::string::npos : dot - a));
                if (dot == std::string::npos) break;
                a = dot + 1;
            }
        sc.field_of[comps] = (uint32_t)f;
        for (size_t k = 0; k <= comps.size(); k++) sc.prefixes.insert(std::vector<std::string>(comps.begin(), comps.begin() + k));
    }
    uint64_t n_leaves = 0, n_text = 0;
    out.rec_off[0] = 0;
    for (uint64_t d = 0; d < n_docs; d++) {
        json::Value v;
        std::vector<RefLeaf> leaves;
        uint32_t status = kJsSyntax;
        if (json::Parse((const char*)blob + doc_off[d], (size_t)(doc_off[d + 1] - doc_off[d]), v).empty()) {
            const uint32_t cond = ref_walk(v, sc, leaves);
            status = cond ? (uint32_t)__builtin_ctz(cond) : (uint32_t)kJsOk;
        }
        out.status[d] = (uint8_t)status;
        if (status == kJsOk)
            for (const RefLeaf& l : leaves) {
                if (n_leaves < out.leaf_cap) { out.leaf_field[n_leaves] = l.field; out.leaf_off[n_leaves] = n_text; }
                for (size_t k = 0; k < l.text->size(); k++)
                    if (n_text + k < out.text_cap) out.text[n_text + k] = (uint8_t)(*l.text)[k];
                n_leaves++;
                n_text += l.text->size();
            }
        out.rec_off[d + 1] = n_leaves;
    }
    if (out.leaf_off && n_leaves <= out.leaf_cap) out.leaf_off[n_leaves] = n_text;
    if (out.totals) { out.totals[0] = n_leaves; out.totals[1] = n_text; }
    return GFT_OK;
}

}  // namespace gft
