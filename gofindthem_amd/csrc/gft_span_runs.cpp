// gft_span_runs.cpp -- the front end the span-run calls share (gft_span_runs.hpp).
#include "gft_span_runs.hpp"

#include <optional>

namespace gft::api {

// what fail_hip names for a step of the call whose word is R.word
static std::string step(const SpanRun& R, const char* what) { return std::string(R.word) + " " + what; }

int span_run_begin(gft_engine* e, ExcerptParams& P, SpanRun& R) {
    hipStream_t st = e->stream;
    auto& X = e->d_excerpt;
    const uint64_t n_docs = P.V.n_docs;
    // the control block and its pinned landing place; the ends of the span list and of the text -- how many lanes the passes get,
    // and what the outputs must not meet -- gathered by one lane and read back in one copy
    if (int rc = room(e, X.ctl, kExcCtlWords * 8, R.room)) return rc;
    if (!X.pin) HIP_TRY(hipHostMalloc((void**)&X.pin, kExcCtlWords * 8, hipHostMallocDefault), "pinned alloc");
    P.ctl = X.ctl.as<uint64_t>();
    HIP_TRY(hipMemsetAsync(P.ctl, 0, kExcCtlWords * 8, st), step(R, "control block").c_str());
    uint64_t ends[4] = {0, 0, 0, 0};
    if (n_docs) {
        HIP_TRY(launch_excerpt_ends(P, st), step(R, "ends kernel launch").c_str());
        HIP_TRY(hipMemcpyAsync(X.pin, P.ctl + kExcCtlEnds, 32, hipMemcpyDeviceToHost, st), "span offsets");
        HIP_TRY(hipStreamSynchronize(st), "span offsets");
        for (int k = 0; k < 4; k++) ends[k] = X.pin[k];
    }
    if (ends[1] < ends[0] || ends[1] - ends[0] > (~0ull >> 4)) return fail(e, GFT_E_INVALID, std::string(R.who) + ": span offsets descend");
    if (ends[3] < ends[2]) return fail(e, GFT_E_INVALID, std::string(R.who) + ": document offsets descend, or a document of 4 GiB or more");
    R.s0 = ends[0]; R.n = ends[1] - ends[0]; R.lo = ends[2]; R.hi = ends[3];
    if (R.n && (!P.V.span_start || !P.V.span_len)) return fail(e, GFT_E_INVALID, "null argument");
    if (R.hi > R.lo && !P.V.text) return fail(e, GFT_E_INVALID, "null argument");
    return GFT_OK;
}

int span_run_room(gft_engine* e, ExcerptParams& P, const SpanRun& R, bool want_pos) {
    auto& X = e->d_excerpt;
    const uint64_t n = R.n, n_tiles = exc_tiles(n);
    int rc;
    if ((rc = room(e, X.ws, n * 8, R.room)) || (rc = room(e, X.we, n * 8, R.room)) || (rc = room(e, X.sdoc, n * 8, R.room)) ||
        (rc = room(e, X.smin, n * 8, R.room)) || (rc = room(e, X.head, n * 4, R.room)) || (rc = room(e, X.share, n * 4, R.room)) ||
        (rc = room(e, X.rank, (n + 1) * 8, R.room)) || (want_pos && (rc = room(e, X.pos, (n + 1) * 8, R.room))) ||
        (rc = room(e, X.tmin, n_tiles * 8, R.room)) || (rc = room(e, X.carry, n_tiles * 8, R.room)) ||
        (rc = room(e, X.partial, scan_partials_needed(std::max<uint64_t>(n, 1)) * 8, R.room)))
        return rc;
    P.s0 = R.s0; P.n_spans = n;
    P.ws = X.ws.as<uint64_t>(); P.we = X.we.as<uint64_t>(); P.sdoc = X.sdoc.as<uint64_t>(); P.smin = X.smin.as<uint64_t>();
    P.tmin = X.tmin.as<uint64_t>(); P.carry = X.carry.as<uint64_t>(); P.head = X.head.as<uint32_t>(); P.share = X.share.as<uint32_t>();
    P.rank = X.rank.as<uint64_t>();
    if (want_pos) P.pos = X.pos.as<uint64_t>();
    return GFT_OK;
}

int span_run_launch(gft_engine* e, const ExcerptParams& P, const SpanRun& R, const char* stage_a, const char* stage_b) {
    hipStream_t st = e->stream;
    std::optional<ProfScope> ps(std::in_place, e, stage_a);
    HIP_TRY(launch_excerpt_docs(P, st), step(R, "document kernel launch").c_str());
    HIP_TRY(launch_excerpt_window(P, st), step(R, "window kernel launch").c_str());
    if (std::strcmp(stage_a, stage_b) != 0) {
        ps.reset();
        ps.emplace(e, stage_b);
    }
    HIP_TRY(launch_excerpt_carry(P, st), step(R, "carry kernel launch").c_str());
    HIP_TRY(launch_excerpt_mark(P, st), (step(R, R.heads) + " kernel launch").c_str());
    return GFT_OK;
}

int span_run_verdict(const gft_engine* e, const SpanRun& R, const uint64_t* h_ctl) {
    if (h_ctl[kExcCtlOffs]) return fail(e, GFT_E_INVALID, std::string(R.who) + ": span offsets descend");
    if (h_ctl[kExcCtlDocs]) return fail(e, GFT_E_INVALID, std::string(R.who) + ": document offsets descend, or a document of 4 GiB or more");
    if (h_ctl[kExcCtlSpans])
        return fail(e, GFT_E_INVALID, std::string(R.who) + ": a span reaches past the end of its document, or the spans' ends descend inside a "
                                                           "document (nothing was written)");
    return GFT_OK;
}

}  // namespace gft::api
