// json_paths.hpp -- the distinct paths of a JSON batch's string values: what the host makes of the state that the discovery
// walk leaves (gft_json.hip: k_json_paths), that walk run on the host, and the reference it is tested against.  Pure: no
// device, no handle (as json_schema.hpp).
#pragma once
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "../../include/gft.h"
#include "gft_json_walk.hpp"

namespace gft {

// the set, the counters and the pool as plain arrays
struct JsonPathState {
    std::vector<uint64_t> slots;
    std::vector<uint32_t> path_off;
    std::unique_ptr<uint8_t[]> pool;               // (not cleared: as on the device)
    uint32_t pool_bytes, count = 0, dropped = 0, cursor = 0;
    explicit JsonPathState(uint32_t pool_bytes_ = kJsonPathPool)
        : slots(kJsonPathSlots, 0), path_off(kJsonPathCap, kJsonNone), pool(new uint8_t[pool_bytes_ ? pool_bytes_ : 1]), pool_bytes(pool_bytes_) {}
    JsonPathSet view() { return JsonPathSet{slots.data(), &count, &dropped, &cursor, path_off.data(), pool.get(), pool_bytes}; }
};

// path numbers 0 .. min(count, kJsonPathCap) - 1 -> their bytes, sorted bytewise, each once.  pool_valid: bytes of the pool
// that were fetched; a number whose path is not wholly inside them is skipped.
void json_paths_collect(uint32_t count, const uint32_t* path_off, const uint8_t* pool, uint64_t pool_valid, std::vector<std::string>& paths);

// the discovery mode of the kernels' walker (gft_json_walk.hpp) on the host, 64-byte piece by piece.  hashes (nullable): the
// values in the set, ascending.  pool_bytes: the pool's size (tests of its overflow may shrink it).
int json_paths_emulate(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, std::vector<std::string>& paths, std::vector<uint64_t>* hashes,
                       uint64_t* dropped, std::string& err, uint32_t pool_bytes = kJsonPathPool);
// json::Parse + a walk that collects every string value's path as a list of components, joined at the end: shares nothing
// with the walker.  Only the documents that json::Parse accepts contribute.
int json_paths_ref(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, std::vector<std::string>& paths, std::string& err);

}  // namespace gft
