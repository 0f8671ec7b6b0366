// group_records.hpp -- GroupFinder::Records, for the three files that work on one: group_records.cpp (the record route),
// group_json.cpp (the JSON routes on top of it) and group_tags.cpp (the tag calls, which ask both for entries instead of rule
// rows).  Not for other includers.
#pragma once
#include "gft_json.hpp"
#include "gft_rules.hpp"
#include "gft_tagdoc.hpp"
#include "gft_tags.hpp"
#include "group_host.hpp"
#include "json_schema.hpp"
#include "rule_set.hpp"
#include "tags_json.hpp"

namespace gft {

struct GroupFinder::Records {
    std::vector<std::string> schema, inc, exc;
    RuleSet set;
    uint64_t rules_version = 0;            // what `set` was compiled from
    size_t n_exprs = 0;
    uint64_t serial = 0;                   // its copy on the engine (rules_install), 0: not uploaded
    JsonSchema json;                       // the schema's component trie (json_schema.hpp) ...
    int json_rc = GFT_OK;                  // ... or why there is none: the JSON calls answer this
    Error json_err;
    uint64_t json_serial = 0;              // its copy on the engine (json_install)
    std::shared_ptr<TagFields> tfields;    // the tag document's field table (tags_json.hpp), made on first use; null when made: refused
    bool tfields_made = false;
    Error tfields_why;
    uint64_t tfields_serial = 0;           // its copy on the engine (tags_json_install)
    uint64_t row_words() const { return (uint64_t)(set.n_rules + 31) / 32; }    // of a rule bitmap row
};

// One of: rule rows [n_records][row_words]; tag entries into the caller's device arrays; tag entries into the engine's own
// arrays (rules_tag_entries_owned), which `owned` then names
struct GroupFinder::RecordsOut {
    uint32_t* d_rule_bitmap = nullptr;
    const TagEntries* d_entries = nullptr;
    struct Owned { const uint64_t* row_off = nullptr; const uint32_t* ent_field = nullptr; const uint32_t* ent_expr = nullptr; uint64_t total = 0; };
    Owned* owned = nullptr;
    // ... or the batch staged for the tag document (tags_json_stage): `tagdoc` then names the kept copy of the record offsets
    struct TagDoc { const uint64_t* d_rec_off = nullptr; };
    TagDoc* tagdoc = nullptr;
    bool tags() const { return d_entries || owned || tagdoc; }
};

struct GroupFinder::JsonStaged {
    std::vector<uint8_t> status;           // [n_docs]
    std::vector<uint32_t> rows;            // rule rows [n_docs][row_words] ...
    std::vector<uint64_t> row_off;         // ... or tag entries: [n_docs + 1], [total], [total]
    std::vector<uint32_t> ent_field, ent_expr;
};

// the finder's engine for a batch on the device, or why there is none (what: "record batches", "JSON batches")
inline int single_device_engine(const Finder* f, const char* what, gft_engine*& e, Error& err) {
    e = f->device_engine();
    if (!e) { err = "no GPU engine"; return GFT_E_HIP; }
    if (gft_n_devices(e) != 1) { err = std::string(what) + ": single-device handles only"; return GFT_E_UNSUPPORTED; }
    return GFT_OK;
}

}  // namespace gft
