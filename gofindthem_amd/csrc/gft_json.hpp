// gft_json.hpp -- JSON documents decoded on the device into the record form (gft_json.hip): parameter block, launchers, and the
// engine's side of it (gft_json_api.cpp) that group_json.cpp drives.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/gft.h"
#include "gft_json_walk.hpp"

namespace gft {

struct JsonSchema;

struct JsonParams {
    const uint8_t* blob;
    const uint64_t* doc_off;     // [n_docs + 1]
    uint64_t n_docs;
    JsonTrie T;                  // device pointers
    uint8_t* status;             // [n_docs]
    uint32_t* cnt_leaves;        // [n_docs]  count pass: written; write pass: read
    uint32_t* cnt_text;          // [n_docs]
    uint32_t* flags;             // [0] |= 1: offsets that descend, or a document of 4 GiB or more
    // write pass
    const uint64_t* rec_off;     // [n_docs + 1]
    const uint64_t* text_off;    // [n_docs + 1]
    uint32_t* leaf_field; uint64_t* leaf_off; uint8_t* text;
    uint64_t leaf_cap, text_cap;
};

struct JsonPathParams {
    const uint8_t* blob;
    const uint64_t* doc_off;     // [n_docs + 1]
    uint64_t n_docs;
    JsonPathSet set;             // device pointers; cleared by the caller
    uint32_t* flags;             // as JsonParams
};

// status, leaves and decoded bytes per document
hipError_t launch_json_count(const JsonParams& P, unsigned n_cus, hipStream_t st);
// the arrays, for the documents of status 0; leaf_off[total leaves] = total text when it lies inside leaf_cap
hipError_t launch_json_write(const JsonParams& P, unsigned n_cus, hipStream_t st);

// discovery: the paths of the batch's string values into P.set
hipError_t launch_json_paths(const JsonPathParams& P, unsigned n_cus, hipStream_t st);

// ---- the engine's side (gft_json_api.cpp); single-device handles only, the calls take the engine's lock (RulesLock around
// several of them, as for the rule kernels)
int json_install(gft_engine* e, const JsonSchema& s, uint64_t* serial);
uint64_t json_serial(gft_engine* e);
// gft_group_json_leaves_device behind the schema's install
int json_leaves_device(gft_engine* e, const uint8_t* d_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint8_t* d_status, uint64_t* d_rec_off,
                       uint32_t* d_leaf_field, uint64_t* d_leaf_off, uint64_t leaf_cap, uint8_t* d_text, uint64_t text_cap, uint64_t* totals);
// the same into buffers the engine owns, grown until the batch fits (64 zero bytes behind the text); the pointers stay valid
// until the next call
int json_leaves_owned(gft_engine* e, const uint8_t* d_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint8_t* d_status,
                      const uint64_t** d_rec_off, const uint32_t** d_leaf_field, const uint64_t** d_leaf_off, const uint8_t** d_text,
                      uint64_t* totals);
// gft_group_json_paths_device: the distinct paths of the batch's string values, sorted bytewise; needs no trie.
int json_paths_device(gft_engine* e, const uint8_t* d_blob, const uint64_t* d_doc_off, uint64_t n_docs, std::vector<std::string>& paths,
                      uint64_t* dropped);
// a batch from host memory into engine-owned buffers (64 zero bytes behind the blob), with room for its status bytes and
// rule bitmap rows
int json_stage(gft_engine* e, const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, uint64_t row_bytes, const uint8_t** d_blob,
               const uint64_t** d_doc_off, uint8_t** d_status, uint32_t** d_rows);
// ... and a blob of JSON Lines: uploaded once, cut into documents where it lies (gft_split_lines_device, GFT_SPLIT_JSON_LINES:
// one call when the offsets fit the buffer kept from earlier batches, else a second one into a larger buffer); h_doc_off receives
// the n_docs + 1 offsets, which the host route needs for the documents the device does not decide
int json_stage_lines(gft_engine* e, const uint8_t* blob, uint64_t len, uint64_t row_bytes, const uint8_t** d_blob, const uint64_t** d_doc_off,
                     uint8_t** d_status, uint32_t** d_rows, std::vector<uint64_t>& h_doc_off);

}  // namespace gft
