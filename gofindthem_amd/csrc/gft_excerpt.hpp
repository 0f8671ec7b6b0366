// gft_excerpt.hpp -- excerpts: the text around the hit spans, cut and gathered (gft_excerpt.hip): the launchers, and the same walk
// on the host (excerpt_host.cpp), which is also what a finder cuts with when it does not take the device route.
#pragma once
#include <stdint.h>

#include "../../include/gft.h"
#include "gft_excerpt_piece.hpp"
#include "gft_select.hpp"

namespace gft {

// gft_excerpt_spans_device's contract on host pointers: the window pass, the carry pass and the mark pass tile by tile, trip by
// trip and lane by lane through gft_excerpt_piece.hpp, the two prefix sums, the place pass, and the copy excerpt by excerpt (the
// device copies with the select's kernel, which select_host.cpp walks).  Reads blob[doc_off[0], doc_off[n_docs]) only and asks
// for no slack.  Returns a gft_status; a refusal writes nothing.
int excerpt_spans_host(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const uint64_t* span_off, const uint32_t* span_start,
                       const uint32_t* span_len, uint32_t before, uint32_t after, uint32_t flags, uint8_t* out, uint64_t cap_bytes,
                       uint64_t* exc_off, uint64_t* exc_doc, uint32_t* exc_start, uint64_t* exc_span_off, uint64_t cap_exc, uint32_t* span_rel,
                       uint64_t* doc_exc_off, uint64_t* n_exc, uint64_t* total_bytes);
// gft_excerpt_spans_snap_device's contract the same way: flags may hold one of GFT_EXCERPT_WORDS / GFT_EXCERPT_LINES, an edge moves
// `reach` bytes at most.  words: the class table the word snap judges by (word_table_host() of gft_words.hpp; not read otherwise)
int excerpt_spans_snap_host(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const uint64_t* span_off, const uint32_t* span_start,
                            const uint32_t* span_len, uint32_t before, uint32_t after, uint32_t flags, uint32_t reach, const WordTable& words,
                            uint8_t* out, uint64_t cap_bytes, uint64_t* exc_off, uint64_t* exc_doc, uint32_t* exc_start, uint64_t* exc_span_off,
                            uint64_t cap_exc, uint32_t* span_rel, uint64_t* doc_exc_off, uint64_t* n_exc, uint64_t* total_bytes);

// an output of the call overlaps one of its inputs (the text is [lo, hi) of the blob, the spans [s0, s0 + n)) or another output
inline bool excerpt_buffers_overlap(const uint8_t* text, uint64_t lo, uint64_t hi, const uint64_t* doc_off, uint64_t n_docs, const uint64_t* span_off,
                                    const uint32_t* span_start, const uint32_t* span_len, uint64_t s0, uint64_t n, const uint8_t* out,
                                    uint64_t cap_bytes, const uint64_t* exc_off, const uint64_t* exc_doc, const uint32_t* exc_start,
                                    const uint64_t* exc_span_off, uint64_t cap_exc, const uint32_t* span_rel, const uint64_t* doc_exc_off) {
    const ByteRange outs[] = {{out, cap_bytes}, {exc_off, (cap_exc + 1) * 8}, {exc_doc, cap_exc * 8}, {exc_start, cap_exc * 4},
                              {exc_span_off, (cap_exc + 1) * 8}, {span_rel ? span_rel + s0 : nullptr, n * 4}, {doc_exc_off, (n_docs + 1) * 8}};
    const ByteRange ins[] = {{text ? text + lo : nullptr, hi > lo ? hi - lo : 0}, {doc_off, (n_docs + 1) * 8}, {span_off, (n_docs + 1) * 8},
                             {span_start ? span_start + s0 : nullptr, n * 4}, {span_len ? span_len + s0 : nullptr, n * 4}};
    return outputs_overlap(outs, ins);
}

}  // namespace gft

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace gft {

// work buffers: 56 bytes per span (ws, we, doc, smin, head, share, rank, pos), 16 per tile, 16 per excerpt
struct ExcerptParams {
    ExcView V;
    uint64_t s0, n_spans;          // the spans [s0, s0 + n_spans) = [span_off[0], span_off[n_docs])
    uint64_t* ws;                  // [n_spans]      window: the snapped window, blob positions
    uint64_t* we;                  // [n_spans]
    uint64_t* sdoc;                // [n_spans]      window: the span's document
    uint64_t* tmin;                // [tiles]        window: the minimum of ws over the tile
    uint64_t* carry;               // [tiles]        carry: the minimum of tmin over the tiles behind this one
    uint64_t* smin;                // [n_spans]      mark: the suffix minimum of ws
    uint32_t* head;                // [n_spans]      mark: 0 / 1
    uint32_t* share;               // [n_spans]      mark: the span's share of its excerpt's length
    const uint64_t* rank;          // [n_spans + 1]  exclusive prefix sum of head
    const uint64_t* pos;           // [n_spans + 1]  ... of share
    uint64_t* ctl;                 // [kExcCtlWords] n_exc, total, the refusals, the ends of the offsets (kExcCtl*)
    uint64_t* c_off;               // [m + 1]        place -> finish, copy
    uint64_t* c_src;               // [m]
    uint64_t m, total;
    uint64_t* exc_off;             // the caller's arrays, each NULL or capped by cap_exc
    uint64_t* exc_doc;
    uint32_t* exc_start;
    uint64_t* exc_span_off;
    uint64_t cap_exc;
    uint32_t* span_rel;            // NULL, or parallel to span_start: entries [s0, s0 + n_spans)
    uint64_t* doc_exc_off;         // NULL, or [n_docs + 1]
};

hipError_t launch_excerpt_ends(const ExcerptParams& P, hipStream_t st);
hipError_t launch_excerpt_docs(const ExcerptParams& P, hipStream_t st);
hipError_t launch_excerpt_window(const ExcerptParams& P, hipStream_t st);
hipError_t launch_excerpt_carry(const ExcerptParams& P, hipStream_t st);
hipError_t launch_excerpt_mark(const ExcerptParams& P, hipStream_t st);
hipError_t launch_excerpt_pack(const ExcerptParams& P, hipStream_t st);
hipError_t launch_excerpt_place(const ExcerptParams& P, hipStream_t st);
hipError_t launch_excerpt_finish(const ExcerptParams& P, hipStream_t st);

}  // namespace gft
#endif
