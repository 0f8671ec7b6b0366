// gft_mark.hpp -- highlight: markers written round the hit spans (gft_mark.hip): the launchers, and the same walk on the host
// (mark_host.cpp).
#pragma once
#include <stdint.h>

#include "../../include/gft.h"
#include "gft_excerpt.hpp"
#include "gft_mark_piece.hpp"
#include "gft_select.hpp"

namespace gft {

// gft_mark_spans_device's contract on host pointers: the runs by the excerpt's host walk (before = after = 0, no snap), the
// insertion list, the index outputs, and the copy tile by tile, trip by trip and lane by lane through gft_mark_piece.hpp.  Reads
// blob[doc_off[0], doc_off[n_docs]) only and asks for no slack.  Returns a gft_status; a refusal writes nothing.
int mark_spans_host(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const uint64_t* span_off, const uint32_t* span_start,
                    const uint32_t* span_len, const uint8_t* open, uint32_t open_len, const uint8_t* close, uint32_t close_len, uint32_t flags,
                    uint8_t* out, uint64_t cap_bytes, uint64_t* out_off, uint32_t* span_new, uint64_t* doc_run_off, uint64_t* n_runs,
                    uint64_t* total_bytes);

// an output of the call overlaps one of its inputs (the text is [lo, hi) of the blob, the spans [s0, s0 + n)) or another output
inline bool mark_buffers_overlap(const uint8_t* text, uint64_t lo, uint64_t hi, const uint64_t* doc_off, uint64_t n_docs, const uint64_t* span_off,
                                 const uint32_t* span_start, const uint32_t* span_len, uint64_t s0, uint64_t n, const uint8_t* out,
                                 uint64_t cap_bytes, const uint64_t* out_off, const uint32_t* span_new, const uint64_t* doc_run_off) {
    const ByteRange outs[] = {{out, cap_bytes}, {out_off, (n_docs + 1) * 8}, {span_new ? span_new + s0 : nullptr, n * 4},
                              {doc_run_off, (n_docs + 1) * 8}};
    const ByteRange ins[] = {{text ? text + lo : nullptr, hi > lo ? hi - lo : 0}, {doc_off, (n_docs + 1) * 8}, {span_off, (n_docs + 1) * 8},
                             {span_start ? span_start + s0 : nullptr, n * 4}, {span_len ? span_len + s0 : nullptr, n * 4}};
    return outputs_overlap(outs, ins);
}

}  // namespace gft

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace gft {

// Work buffers: the excerpt's per span (ws, we, doc, smin 8 bytes each, head, share 4 each, rank 8: 48 bytes per span, 16 per
// tile of kExcTile spans) and 16 bytes per run (the insertion list), 528 for the markers.
struct MarkParams {
    ExcerptParams X;               // the run passes are the excerpt's: V, s0, n_spans, ws .. rank, ctl
    MarkPlan M;                    // q is written by the place pass and read by the copy
    uint64_t* q;
    const uint64_t* marks;         // [kMarkWords] the marker block on the device
    uint64_t* out_off;             // the caller's arrays, each NULL or complete
    uint32_t* span_new;
    uint64_t* doc_run_off;
    uint8_t* out;
    SelGeom G;
};

hipError_t launch_mark_check(const MarkParams& P, hipStream_t st);
hipError_t launch_mark_place(const MarkParams& P, hipStream_t st);
hipError_t launch_mark_copy(const MarkParams& P, hipStream_t st);

}  // namespace gft
#endif
