// json_paths.cpp -- the distinct paths of a JSON batch's string values (json_paths.hpp).  No device, no handle.
#include "json_paths.hpp"

#include <algorithm>
#include <cstring>
#include <memory>

#include "json_host_wave.hpp"
#include "json_mini.hpp"
#include "json_schema.hpp"

namespace gft {

void json_paths_collect(uint32_t count, const uint32_t* path_off, const uint8_t* pool, uint64_t pool_valid, std::vector<std::string>& paths) {
    paths.clear();
    const uint32_t n = std::min(count, kJsonPathCap);
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t off = path_off[i];
        if (off == kJsonNone || off + 4 > pool_valid) continue;
        uint32_t len;
        memcpy(&len, pool + off, 4);
        if (len > kJsonPathMax || off + 4 + len > pool_valid) continue;
        paths.emplace_back((const char*)pool + off + 4, len);
    }
    std::sort(paths.begin(), paths.end());
    paths.erase(std::unique(paths.begin(), paths.end()), paths.end());
}

int json_paths_emulate(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, std::vector<std::string>& paths, std::vector<uint64_t>* hashes,
                       uint64_t* dropped, std::string& err, uint32_t pool_bytes) {
    if (n_docs && (!blob || !doc_off)) { err = "JSON batch: null argument"; return GFT_E_INVALID; }
    int rc = json_check_offsets(doc_off, n_docs, err);
    if (rc) return rc;
    JsonPathState st(pool_bytes);
    auto mem = std::make_unique<JsonWaveMem>();
    auto pm = std::make_unique<JsonPathMem>();
    HostWave w;
    w.m = mem.get();
    JsonPaths dsc{pm.get(), st.view()};
    for (uint64_t d = 0; d < n_docs; d++) json_walk_paths(w, dsc, blob + doc_off[d], (uint32_t)(doc_off[d + 1] - doc_off[d]));
    json_paths_collect(st.count, st.path_off.data(), st.pool.get(), std::min<uint64_t>(st.cursor, st.pool_bytes), paths);
    if (dropped) *dropped = st.dropped;
    if (hashes) {
        hashes->clear();
        for (uint64_t v : st.slots) if (v) hashes->push_back(v);
        std::sort(hashes->begin(), hashes->end());
    }
    return GFT_OK;
}

int json_paths_ref(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, std::vector<std::string>& paths, std::string& err) {
    if (n_docs && (!blob || !doc_off)) { err = "JSON batch: null argument"; return GFT_E_INVALID; }
    int rc = json_check_offsets(doc_off, n_docs, err);
    if (rc) return rc;
    paths.clear();
    struct Item { const json::Value* v; std::vector<std::string> comps; };
    for (uint64_t d = 0; d < n_docs; d++) {
        json::Value root;
        if (!json::Parse((const char*)blob + doc_off[d], (size_t)(doc_off[d + 1] - doc_off[d]), root).empty()) continue;
        std::vector<Item> todo;
        todo.push_back(Item{&root, {}});
        while (!todo.empty()) {
            Item it = std::move(todo.back());
            todo.pop_back();
            const json::Value& v = *it.v;
            if (v.kind == json::Value::String) {
                std::string p;
                for (size_t k = 0; k < it.comps.size(); k++) { if (k) p += '.'; p += it.comps[k]; }
                if (p.size() <= kJsonPathMax) paths.push_back(std::move(p));
                continue;
            }
            if (v.kind != json::Value::Object && v.kind != json::Value::Array) continue;
            if (it.comps.size() >= kJsonMaxDepth) continue;                // its members lie below 32 containers
            if (v.kind == json::Value::Object) {
                for (const auto& m : v.obj) {                              // (a repeated key's earlier values too, as the walker)
                    if (m.first.empty() || (m.second.key_flags & (json::Value::kRawEscape | json::Value::kRawInvalidUtf8))) continue;
                    Item kid{&m.second, it.comps};
                    kid.comps.push_back(m.first);
                    todo.push_back(std::move(kid));
                }
            } else {
                for (size_t i = 0; i < v.arr.size(); i++) {
                    Item kid{&v.arr[i], it.comps};
                    kid.comps.push_back("index(" + std::to_string(i) + ")");
                    todo.push_back(std::move(kid));
                }
            }
        }
    }
    std::sort(paths.begin(), paths.end());
    paths.erase(std::unique(paths.begin(), paths.end()), paths.end());
    return GFT_OK;
}

}  // namespace gft
