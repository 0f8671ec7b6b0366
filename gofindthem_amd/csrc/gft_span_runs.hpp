// gft_span_runs.hpp -- the front end the span-run calls share (excerpts, highlight, replace): the ends of the span list and of the
// text read back, the work buffers of the run passes, the four run launches of gft_excerpt.hip, and the refusals those passes
// leave in the control block.  All in e->d_excerpt, on an ExcerptParams whose V the caller has filled.  A call goes: begin, its own
// overlap check (which needs the ends), room, its own buffers and uploads, launch, its own scans and checks and its own read-back of
// the control block into e->d_excerpt.pin, verdict, its own refusals, place and copy.  It owns the SyncOnExit: the host memory the
// asynchronous copies read is the entry point's.
#pragma once
#include "gft_engine.hpp"
#include "gft_excerpt.hpp"

namespace gft::api {

struct SpanRun {
    const char* who;               // the entry point the refusals name
    const char* word;              // the call's word in what fail_hip names: "<word> ends kernel launch", ...
    const char* heads;             // ... and its word for the fourth run pass: "<word> <heads> kernel launch"
    RoomTexts room;
    uint64_t s0 = 0, n = 0;        // begin: the spans are [s0, s0 + n)
    uint64_t lo = 0, hi = 0;       // begin: the text is [lo, hi) of the blob
};

// Room for the control block and its pinned landing place, the block cleared; with documents the ends pass and its read-back (one
// synchronisation).  Refuses ends that descend and the arrays they make necessary when those are null; fills R.s0 .. R.hi.
int span_run_begin(gft_engine* e, ExcerptParams& P, SpanRun& R);
// room for the per-span and per-tile buffers of the run passes (pos: only for a call that scans the shares), wired into P
int span_run_room(gft_engine* e, ExcerptParams& P, const SpanRun& R, bool want_pos);
// the four run launches: documents and windows under stage_a, carry and heads under stage_b (the same name: one stage)
int span_run_launch(gft_engine* e, const ExcerptParams& P, const SpanRun& R, const char* stage_a, const char* stage_b);
// what the run passes refuse, from the control words the caller has read back
int span_run_verdict(const gft_engine* e, const SpanRun& R, const uint64_t* h_ctl);

}  // namespace gft::api
