// gft_spans.hpp -- hit spans and redaction (gft_spans.hip): the launchers, and the same walks on the host (spans_host.cpp).
#pragma once
#include <stdint.h>

#include "../../include/gft.h"
#include "gft_select.hpp"
#include "gft_spans_piece.hpp"

namespace gft {

// gft_hit_spans_device behind its scan, on host pointers: the mark pass, the prefix sum and the place pass over a match CSR, match
// tile by match tile through gft_spans_piece.hpp.  term_len [n_terms]; wit_off / wit_expr: the witness table; bitmap rows of
// ceil(n_exprs / 32) words.  Returns a gft_status.
int hit_spans_host(const uint64_t* match_off, const uint32_t* term_id, const uint32_t* pos, uint64_t n_docs, const uint32_t* term_len,
                   uint32_t pos_end, const uint64_t* wit_off, const uint32_t* wit_expr, const uint32_t* bitmap, uint32_t n_exprs,
                   const uint64_t* row_idx, const uint32_t* want, uint64_t* span_off, uint32_t* span_start, uint32_t* span_len,
                   uint32_t* span_term, uint64_t cap, uint64_t* total);

// gft_redact_spans_device on host pointers: the check pass, then the fill pass tile by tile and lane by lane.
int redact_spans_host(uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const uint64_t* span_off, const uint32_t* span_start,
                      const uint32_t* span_len, uint32_t mask_byte);

// an output of a spans call (span_off [n_docs + 1], three arrays of cap words) overlaps one of the n_in input ranges, or another
inline bool spans_outputs_overlap(const uint64_t* span_off, uint64_t n_docs, const uint32_t* s0, const uint32_t* s1, const uint32_t* s2, uint64_t cap,
                                  const ByteRange* ins, size_t n_in) {
    const ByteRange outs[] = {{span_off, span_off ? (n_docs + 1) * 8 : 0}, {s0, cap * 4}, {s1, cap * 4}, {s2, cap * 4}};
    return outputs_overlap(outs, 4, ins, n_in);
}

}  // namespace gft

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace gft {

struct SpanParams {
    const uint64_t* match_off;     // [n_docs + 1]   the scan's canonical CSR
    const uint32_t* term;          // [n_matches]
    const uint32_t* pos;           // [n_matches]
    uint64_t n_docs, n_matches;
    const uint32_t* term_len;      // [n_terms]
    uint32_t pos_end;
    const uint64_t* wit_off;       // [n_terms + 1]  the witness table
    const uint32_t* wit_expr;
    const uint32_t* bitmap;        // rows of W words
    uint32_t W;
    const uint64_t* row_idx;       // [n_docs] or NULL: the row of document d
    const uint32_t* want;          // [W], the engine's copy, or NULL: every expression
    uint32_t* keep;                // [n_matches]      mark
    const uint64_t* rank;          // [n_matches + 1]  exclusive prefix sum of keep
    uint64_t* span_off;            // [n_docs + 1] or NULL
    uint32_t* span_start;          // [cap] or NULL
    uint32_t* span_len;
    uint32_t* span_term;
    uint64_t cap;
};

struct RedactParams {
    uint8_t* text;
    const uint64_t* doc_off;       // [n_docs + 1]
    uint64_t n_docs;
    const uint64_t* span_off;      // [n_docs + 1]
    const uint32_t* span_start;
    const uint32_t* span_len;
    uint64_t s0, n_spans;          // the spans [s0, s0 + n_spans) = [span_off[0], span_off[n_docs])
    uint64_t* dst;                 // [n_spans]   check: where the span's first byte lies in the text
    uint32_t* ctl;                 // [1]         check: a span reaches past its document
    uint32_t mask;
};

hipError_t launch_span_mark(const SpanParams& P, unsigned n_cus, hipStream_t st);
hipError_t launch_span_place(const SpanParams& P, hipStream_t st);
hipError_t launch_redact_check(const RedactParams& P, hipStream_t st);
hipError_t launch_redact_fill(const RedactParams& P, hipStream_t st);

}  // namespace gft
#endif
