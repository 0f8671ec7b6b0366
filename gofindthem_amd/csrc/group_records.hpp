// group_records.hpp -- GroupFinder::Records, for the two files that work on one: group_records.cpp (the record route) and
// group_json.cpp (the JSON routes on top of it).  Not for other includers.
#pragma once
#include "gft_json.hpp"
#include "gft_rules.hpp"
#include "group_host.hpp"
#include "json_schema.hpp"
#include "rule_set.hpp"

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
    uint64_t row_words() const { return (uint64_t)(set.n_rules + 31) / 32; }    // of a rule bitmap row
};

// the finder's engine for a batch on the device, or why there is none (what: "record batches", "JSON batches")
inline int single_device_engine(const Finder* f, const char* what, gft_engine*& e, Error& err) {
    e = f->device_engine();
    if (!e) { err = "no GPU engine"; return GFT_E_HIP; }
    if (gft_n_devices(e) != 1) { err = std::string(what) + ": single-device handles only"; return GFT_E_UNSUPPORTED; }
    return GFT_OK;
}

}  // namespace gft
