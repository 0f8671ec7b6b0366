// gft_lowermap.hpp -- spans of a lowered batch mapped back to the source text (gft_lowermap.hip): the launchers, and the same
// walk on the host (lowermap_host.cpp).
#pragma once
#include <stdint.h>

#include "../../include/gft.h"
#include "gft_tolower.hpp"
#include "gft_lowermap_piece.hpp"
#include "gft_spans_piece.hpp"

namespace gft {

// gft_map_spans_to_source_device on host pointers: the unit table, the count pass and the table pass unit by unit and piece by
// piece, then the check and the write pass span tile by span tile, through the headers the kernels compile.  blob must be readable
// 64 bytes past doc_off[n_docs].  Spans at and past `limit` (an index into the span arrays) are left alone.
int lowermap_host(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const uint64_t* span_off, uint32_t* span_start,
                  uint32_t* span_len, uint64_t limit);

struct LowerMapParams {
    LowerMapView V;
    const uint64_t* span_off;      // [n_docs + 1]
    uint32_t* span_start;
    uint32_t* span_len;
    uint64_t s0, n_spans;          // the spans [s0, s0 + n_spans): from span_off[0] to span_off[n_docs] or the limit
    uint32_t* mapped;              // [2 n_spans]  check: (source start, source length)
    uint32_t* ctl;                 // [1]          check: a span reaches past its document's lowered end
};

hipError_t launch_lowermap_check(const LowerMapParams& P, hipStream_t st);
hipError_t launch_lowermap_write(const LowerMapParams& P, hipStream_t st);

}  // namespace gft

// for finder_host.cpp: gft_map_spans_to_source_device over the spans below `limit` only -- what a capped gft_hit_spans_device wrote
extern "C" int gft_map_spans_limit(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs,
                                   const uint64_t* d_span_off, uint32_t* d_span_start, uint32_t* d_span_len, uint64_t limit);
