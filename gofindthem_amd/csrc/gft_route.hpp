// gft_route.hpp -- documents routed to per-bucket runs of one blob (gft_route.hip): the launchers, and the same walk on the host
// (route_host.cpp), which is also what a finder routes with when it does not take the device route.
#pragma once
#include <stdint.h>

#include "../../include/gft.h"
#include "gft_route_piece.hpp"
#include "gft_select.hpp"

namespace gft {

// gft_route_docs_device's contract on host pointers: mark, count, the prefix sum of the counts, place, the prefix sum of the
// entry lengths and the select's copy walk, tile by tile through gft_route_piece.hpp.  Returns a gft_status.
int route_docs_host(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const uint32_t* bitmap, uint32_t n_cols,
                    const uint32_t* masks, uint32_t n_buckets, uint32_t mode, uint32_t flags, const uint8_t* also, uint8_t* out,
                    uint64_t cap_bytes, uint64_t* out_off, uint64_t* doc_idx, uint64_t cap_docs, uint64_t* bucket_doc, uint64_t* bucket_byte);

// the masks as the mark pass reads them: n_buckets rows of W = ceil(n_cols / 32) words, the bits at and above n_cols cleared
inline void route_mask_words(const uint32_t* masks, uint32_t n_buckets, uint32_t n_cols, uint32_t* dst) {
    const uint32_t W = (n_cols + 31) / 32;
    for (uint32_t k = 0; k < n_buckets; k++) {
        for (uint32_t j = 0; j < W; j++) dst[k * W + j] = masks[k * W + j];
        if (W && (n_cols & 31)) dst[k * W + W - 1] &= (1u << (n_cols & 31)) - 1;
    }
}

// the words of the control block the host reads back: the entries, the bytes, the text's range, the flag, then the B + 1 bucket
// borders in entries and -- with the final synchronisation -- in bytes.  The range and the flag lie where the select has them: the
// shared read-back (gft_doc_gather.hpp) looks there
enum : uint32_t {
    kRouteCtlM = 0, kRouteCtlTotal = 1, kRouteCtlLo = kSelCtlLo, kRouteCtlHi = kSelCtlHi, kRouteCtlFlag = kSelCtlFlag, kRouteCtlDoc = 5,
    kRouteCtlByte = kRouteCtlDoc + GFT_ROUTE_MAX_BUCKETS + 1, kRouteCtlWords = kRouteCtlByte + GFT_ROUTE_MAX_BUCKETS + 1
};

// an output of the call overlaps one of its inputs (the text is [lo, hi) of the blob), or another output: select_buffers_overlap
// with the masks among the inputs and the two bucket arrays among the outputs
inline bool route_buffers_overlap(const uint8_t* text, uint64_t lo, uint64_t hi, const uint64_t* doc_off, uint64_t n_docs,
                                  const uint32_t* bitmap, uint32_t n_cols, const uint32_t* masks, uint32_t n_buckets, const uint8_t* also,
                                  const uint8_t* out, uint64_t cap_bytes, const uint64_t* out_off, const uint64_t* doc_idx, uint64_t cap_docs,
                                  const uint64_t* bucket_doc, const uint64_t* bucket_byte, uint32_t B) {
    const uint64_t W = (n_cols + 31) / 32;
    const ByteRange outs[] = {{out, cap_bytes}, {out_off, out_off ? (cap_docs + 1) * 8 : 0}, {doc_idx, cap_docs * 8},
                              {bucket_doc, (uint64_t)(B + 1) * 8}, {bucket_byte, (uint64_t)(B + 1) * 8}};
    const ByteRange ins[] = {{text ? text + lo : nullptr, hi > lo ? hi - lo : 0}, {doc_off, (n_docs + 1) * 8}, {bitmap, n_docs * W * 4},
                             {also, n_docs}, {masks, n_buckets * W * 4}};
    return outputs_overlap(outs, ins);
}

}  // namespace gft

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace gft {

struct RouteParams {
    const uint64_t* doc_off;   // [n_docs + 1]
    uint64_t n_docs, n_tiles;
    const uint32_t* bitmap;    // [n_docs][W]
    uint32_t W, lg;            // words per row; W <= 64: a row is a segment of 1 << lg lanes
    uint32_t n_buckets, B;     // masks; buckets, the rest bucket included
    uint32_t mode, rest;
    const uint32_t* masks;     // [n_buckets][W]    the engine's copy, cut to n_cols
    const uint8_t* also;       // [n_docs] or NULL
    uint64_t* member;          // [n_docs]          mark: bit b = an entry in bucket b
    uint32_t* len;             // [n_docs]          mark: the document's length
    uint32_t* cnt;             // [B * n_tiles]     count: entries of bucket b in a tile, bucket-major
    uint64_t* tile_bytes;      // [n_tiles]         count: bytes of a tile's entries
    const uint64_t* base;      // [B * n_tiles + 1] exclusive prefix sum of cnt
    uint64_t* ctl;             // [kRouteCtlWords]
    uint32_t* ent_len;         // [m]               place: an entry's length
    uint64_t* c_src;           // [m]               place: where its document starts in the text
    const uint64_t* c_off;     // [m + 1]           exclusive prefix sum of ent_len: where it starts in the output
    uint64_t m;
    uint64_t* out_off;         // [cap_docs + 1] or NULL
    uint64_t* doc_idx;         // [cap_docs]
    uint64_t cap_docs;
};

hipError_t launch_route_mark(const RouteParams& P, unsigned n_cus, hipStream_t st);
hipError_t launch_route_count(const RouteParams& P, unsigned n_cus, hipStream_t st);
hipError_t launch_route_pack(const RouteParams& P, hipStream_t st);
hipError_t launch_route_place(const RouteParams& P, unsigned n_cus, hipStream_t st);
hipError_t launch_route_finish(const RouteParams& P, hipStream_t st);

}  // namespace gft
#endif
