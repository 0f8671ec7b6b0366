// json_schema.hpp -- the schema of a record batch as a component trie, for the device JSON walker (gft_json.hip) and its
// host emulation.  Pure: no device, no handle (as rule_set.hpp).
//
// Every schema path is split at '.' into components; the root node is the path "".  A node maps to a field index when its
// path is a schema path.  (parent node, key bytes) -> child goes through an open-addressing table whose hit is confirmed by
// comparing the key bytes (gft_json_walk.hpp: trie_find); an array element i is looked up as the component "index(<i>)", so
// the object key "index(2)" and array element 2 reach the same node, as they give the same path string in the reference.
// A key that contains '.' never resolves.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/gft.h"
#include "gft_json_walk.hpp"

namespace gft {

struct JsonSchema {
    std::vector<JsonTrieNode> nodes;               // [0] is the root
    std::vector<uint8_t> keys;                     // the components' bytes, 64 bytes of slack behind them
    std::vector<uint32_t> table;                   // open addressing, kJsonNone: empty; size is a power of two
    uint32_t n_fields = 0;
    uint32_t max_key_len = 0;
    JsonTrie view() const {
        return JsonTrie{nodes.data(), keys.data(), table.data(), (uint32_t)table.size() - 1, (uint32_t)nodes.size(), max_key_len};
    }
};

// GFT_E_UNSUPPORTED names the limit (more than kJsonMaxNodes nodes, a component longer than kJsonMaxKey)
int compile_json_schema(const std::vector<std::string>& paths, JsonSchema& out, std::string& err);
// child of `parent` under the component `key`, or kJsonNone (the walker's own lookup run over host arrays)
uint32_t json_schema_find(const JsonSchema& s, uint32_t parent, const uint8_t* key, uint32_t len);

// The arrays of gft_group_json_leaves_device, host pointers: status [n_docs], rec_off [n_docs + 1], leaf_field [leaf_cap],
// leaf_off [leaf_cap + 1], text [text_cap]; NULL arrays with zero caps count only; totals[2] = leaves, text bytes.
struct JsonLeavesOut {
    uint8_t* status; uint64_t* rec_off; uint32_t* leaf_field; uint64_t* leaf_off; uint64_t leaf_cap; uint8_t* text; uint64_t text_cap;
    uint64_t* totals;
};
// GFT_E_INVALID + err: descending offsets, a document of 4 GiB or more
int json_check_offsets(const uint64_t* doc_off, uint64_t n_docs, std::string& err);
// json::Parse + a walk of the decoded value against the schema, classified into the gft_json_status values: shares nothing
// with the walker below
int json_leaves_ref(const std::vector<std::string>& paths, const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs,
                    const JsonLeavesOut& out, std::string& err);
// the kernels' walker (gft_json_walk.hpp) on the host, 64-byte piece by piece: count, prefix sums, write
int json_leaves_emulate(const JsonSchema& s, const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const JsonLeavesOut& out,
                        std::string& err);

}  // namespace gft
