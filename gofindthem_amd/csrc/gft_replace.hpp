// gft_replace.hpp -- replace: every hit run rewritten by its replacement (gft_replace.hip): the launchers, and the same walk on
// the host (replace_host.cpp).
#pragma once
#include <stdint.h>

#include "../../include/gft.h"
#include "gft_excerpt.hpp"
#include "gft_replace_piece.hpp"
#include "gft_select.hpp"

namespace gft {

// gft_replace_spans_device's contract on host pointers: the runs by the excerpt's host walk (before = after = 0, no snap), every
// run's smallest id, the plan, the index outputs, and the copy tile by tile, trip by trip and lane by lane through
// gft_replace_piece.hpp.  Reads blob[doc_off[0], doc_off[n_docs]) only and asks for no slack.  Returns a gft_status; a refusal
// writes nothing.
int replace_spans_host(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const uint64_t* span_off, const uint32_t* span_start,
                       const uint32_t* span_len, const uint32_t* span_key, const uint32_t* key_rep, uint32_t n_keys, const uint8_t* rep_bytes,
                       const uint64_t* rep_off, uint32_t n_reps, uint32_t flags, uint8_t* out, uint64_t cap_bytes, uint64_t* out_off,
                       uint64_t* doc_run_off, uint32_t* run_new, uint32_t* run_len, uint32_t* run_rep, uint64_t cap_runs, uint64_t* n_runs,
                       uint64_t* total_bytes);

// the table is well formed: 1 .. kRepMaxReps entries, rep_off[0] == 0, ascending, no entry longer than GFT_REPLACE_MAX
inline bool replace_table_ok(const uint8_t* rep_bytes, const uint64_t* rep_off, uint32_t n_reps) {
    if (!n_reps || n_reps > kRepMaxReps || !rep_off || rep_off[0]) return false;
    for (uint32_t k = 0; k < n_reps; k++)
        if (rep_off[k + 1] < rep_off[k] || rep_off[k + 1] - rep_off[k] > GFT_REPLACE_MAX) return false;
    return rep_off[n_reps] == 0 || rep_bytes;
}

// an output of the call overlaps one of its inputs (the text is [lo, hi) of the blob, the spans [s0, s0 + n)) or another output
inline bool replace_buffers_overlap(const uint8_t* text, uint64_t lo, uint64_t hi, const uint64_t* doc_off, uint64_t n_docs, const uint64_t* span_off,
                                    const uint32_t* span_start, const uint32_t* span_len, const uint32_t* span_key, uint64_t s0, uint64_t n,
                                    const uint8_t* out, uint64_t cap_bytes, const uint64_t* out_off, const uint64_t* doc_run_off,
                                    const uint32_t* run_new, const uint32_t* run_len, const uint32_t* run_rep, uint64_t cap_runs) {
    const ByteRange outs[] = {{out, cap_bytes}, {out_off, (n_docs + 1) * 8}, {doc_run_off, (n_docs + 1) * 8}, {run_new, cap_runs * 4},
                              {run_len, cap_runs * 4}, {run_rep, cap_runs * 4}};
    const ByteRange ins[] = {{text ? text + lo : nullptr, hi > lo ? hi - lo : 0}, {doc_off, (n_docs + 1) * 8}, {span_off, (n_docs + 1) * 8},
                             {span_start ? span_start + s0 : nullptr, n * 4}, {span_len ? span_len + s0 : nullptr, n * 4},
                             {span_key ? span_key + s0 : nullptr, n * 4}};
    return outputs_overlap(outs, ins);
}

}  // namespace gft

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace gft {

// Work buffers: the excerpt's per span (ws, we, doc, smin, rank, pos 8 bytes each, head, share 4 each: 56 bytes per span, 16 per
// tile of kExcTile spans), 16 more per span of this call's own (rid, pl 4 each, ppos 8), 24 per run (the plan), and the table:
// its bytes, 8 per entry, 4 per key.
struct ReplaceParams {
    ExcerptParams X;               // the run passes are the excerpt's: V, s0, n_spans, ws .. rank, pos, ctl
    const uint32_t* span_key;      // the caller's, nullable
    const uint32_t* key_rep;       // the call's copy on the device, nullable
    uint32_t n_keys, n_reps;
    const uint64_t* rep_off;       // [n_reps + 1] the call's copy on the device
    const uint8_t* tab;            // [tab_bytes + kRepTableSlack or more] ...
    uint32_t tab_bytes;
    uint32_t* rid;                 // [n_spans] ids: entry r is the smallest id of run r
    uint32_t* pl;                  // [n_spans] len: at a head the bytes of its run's replacement, else 0
    const uint64_t* ppos;          // [n_spans + 1] exclusive prefix sum of pl
    uint64_t text_len;             // doc_off[n_docs] - doc_off[0]
    RepPlan R;                     // written by the place pass (the four pointers below) and read by the copy
    uint64_t* at;
    uint64_t* delta;
    uint32_t* len;
    uint32_t* roff;
    uint64_t* out_off;             // the caller's arrays, each NULL or complete
    uint64_t* doc_run_off;
    uint32_t* run_new;             // ... each NULL or capped by cap_runs
    uint32_t* run_len;
    uint32_t* run_rep;
    uint64_t cap_runs;
    uint8_t* out;
    SelGeom G;
};

hipError_t launch_replace_ids(const ReplaceParams& P, hipStream_t st);
hipError_t launch_replace_len(const ReplaceParams& P, hipStream_t st);
hipError_t launch_replace_check(const ReplaceParams& P, hipStream_t st);
hipError_t launch_replace_place(const ReplaceParams& P, hipStream_t st);
hipError_t launch_replace_copy(const ReplaceParams& P, hipStream_t st);

}  // namespace gft
#endif
