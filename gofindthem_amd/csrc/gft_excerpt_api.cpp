// gft_excerpt_api.cpp -- excerpts: the text around the hit spans, cut and gathered (gft_excerpt.hip, the copy pass of
// gft_select.hip): gft_excerpt_spans_device, gft_excerpt_spans_snap_device (the windows snapped to word or line borders), and the
// host walk behind gft_debug_excerpt_spans / gft_debug_excerpt_spans_snap / gft_debug_excerpt_snap_edges.
#include "gft_doc_gather.hpp"
#include "gft_engine.hpp"
#include "gft_excerpt.hpp"
#include "gft_span_runs.hpp"
#include "gft_words.hpp"

using namespace gft;
using namespace gft::api;

namespace {
constexpr RoomTexts kExcRoom{"no device memory for the excerpts' work buffers", "excerpt alloc"};
const char kWhoPlain[] = "gft_excerpt_spans_device";
const char kWhoSnap[] = "gft_excerpt_spans_snap_device";

// both calls behind the lock and their own checks of flags and reach (reach 0 and no snap bit: the plain call)
int excerpt_run(gft_engine* e, const char* kWho, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs, const uint64_t* d_span_off,
                const uint32_t* d_span_start, const uint32_t* d_span_len, uint32_t before, uint32_t after, uint32_t flags, uint32_t reach,
                uint8_t* d_out, uint64_t cap_bytes, uint64_t* d_exc_off, uint64_t* d_exc_doc, uint32_t* d_exc_start, uint64_t* d_exc_span_off,
                uint64_t cap_exc, uint32_t* d_span_rel, uint64_t* d_doc_exc_off, uint64_t* n_exc, uint64_t* total_bytes) {
    if (n_docs && (!d_doc_off || !d_span_off)) return fail(e, GFT_E_INVALID, "null argument");
    if (cap_bytes && !d_out) return fail(e, GFT_E_INVALID, std::string(kWho) + ": cap_bytes but no output buffer");
    if (!e->peers.empty()) return fail(e, GFT_E_UNSUPPORTED, std::string(kWho) + ": single-device handles only");
    int rc = check_ready(e, kNeedDevice | kNeedSettled, kWho);
    if (rc) return rc;
    if (cap_exc > (~0ull >> 4) || n_docs > (~0ull >> 4)) return fail(e, GFT_E_INVALID, std::string(kWho) + ": a size beyond the address space");
    DeviceGuard g(e->device);
    hipStream_t st = e->stream;
    auto& X = e->d_excerpt;
    SyncOnExit drain(e);                                            // (the pinned words are handed to asynchronous copies)
    ExcerptParams P{};
    P.V = ExcView{d_text_blob, d_doc_off, n_docs, d_span_off, d_span_start, d_span_len, before, after, flags};
    if (flags & GFT_EXCERPT_WORDS) {
        if ((rc = ensure_word_table(e))) return rc;
        P.V.words = WordTable{e->d_words.tab_row.as<uint16_t>(), e->d_words.tab_bits.as<uint32_t>()};
    }
    P.V.reach = reach;
    SpanRun R{kWho, "excerpt", "mark", kExcRoom};
    if ((rc = span_run_begin(e, P, R))) return rc;
    const uint64_t n = R.n;
    if (excerpt_buffers_overlap(d_text_blob, R.lo, R.hi, d_doc_off, n_docs, d_span_off, d_span_start, d_span_len, R.s0, n, d_out, cap_bytes,
                                d_exc_off, d_exc_doc, d_exc_start, d_exc_span_off, cap_exc, d_span_rel, d_doc_exc_off))
        return fail(e, GFT_E_INVALID, std::string(kWho) + ": an output overlaps an input or another output");
    if ((rc = span_run_room(e, P, R, true)) || (rc = span_run_launch(e, P, R, "excerpt_window", "excerpt_smin"))) return rc;
    if (n) {
        ProfScope ps(e, "excerpt_scan");
        HIP_TRY(launch_exclusive_scan(P.head, n, X.rank.as<uint64_t>(), X.partial.as<uint64_t>(), st), "excerpt scan");
        HIP_TRY(launch_exclusive_scan(P.share, n, X.pos.as<uint64_t>(), X.partial.as<uint64_t>(), st), "excerpt scan");
        HIP_TRY(launch_excerpt_pack(P, st), "excerpt scan");
    } else {
        HIP_TRY(hipMemsetAsync(X.rank.p, 0, 8, st), "excerpt scan");    // (no span: rank[0] is what the finish pass reads)
    }
    const uint64_t* h_ctl = X.pin;
    HIP_TRY(hipMemcpyAsync(X.pin, P.ctl, (kExcCtlOffs + 1) * 8, hipMemcpyDeviceToHost, st), "excerpt totals");
    HIP_TRY(hipStreamSynchronize(st), "excerpt totals");
    if ((rc = span_run_verdict(e, R, h_ctl))) return rc;
    P.m = h_ctl[kExcCtlExc]; P.total = h_ctl[kExcCtlTotal];
    if (n_exc) *n_exc = P.m;
    if (total_bytes) *total_bytes = P.total;
    if ((rc = room(e, X.c_off, (P.m + 1) * 8, kExcRoom)) || (rc = room(e, X.c_src, P.m * 8, kExcRoom))) return rc;
    P.c_off = X.c_off.as<uint64_t>(); P.c_src = X.c_src.as<uint64_t>();
    P.exc_off = d_exc_off; P.exc_doc = d_exc_doc; P.exc_start = d_exc_start; P.exc_span_off = d_exc_span_off; P.cap_exc = cap_exc;
    P.span_rel = d_span_rel; P.doc_exc_off = n_docs ? d_doc_exc_off : nullptr;
    {
        ProfScope ps(e, "excerpt_place");
        HIP_TRY(launch_excerpt_place(P, st), "excerpt place kernel launch");
        HIP_TRY(launch_excerpt_finish(P, st), "excerpt finish kernel launch");
        if (!n_docs && d_doc_exc_off) HIP_TRY(hipMemsetAsync(d_doc_exc_off, 0, 8, st), "excerpt offsets");
    }
    // the select's copy pass over the excerpts
    if ((rc = select_copy_run(e, d_text_blob, P.c_off, P.c_src, P.m, P.total, d_out, cap_bytes, "excerpt_copy", "excerpt copy kernel launch")))
        return rc;
    HIP_TRY(hipStreamSynchronize(st), "excerpt copy");
    return GFT_OK;
}
}  // namespace

extern "C" {

int gft_excerpt_spans_device(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs,
                             const uint64_t* d_span_off, const uint32_t* d_span_start, const uint32_t* d_span_len, uint32_t before,
                             uint32_t after, uint32_t flags, uint8_t* d_out, uint64_t cap_bytes, uint64_t* d_exc_off, uint64_t* d_exc_doc,
                             uint32_t* d_exc_start, uint64_t* d_exc_span_off, uint64_t cap_exc, uint32_t* d_span_rel,
                             uint64_t* d_doc_exc_off, uint64_t* n_exc, uint64_t* total_bytes) try {
    if (!e) return GFT_E_INVALID;
    GFT_LOCK(e);
    if (n_exc) *n_exc = 0;
    if (total_bytes) *total_bytes = 0;
    if (flags & ~(uint32_t)GFT_EXCERPT_RUNES) return fail(e, GFT_E_INVALID, std::string(kWhoPlain) + ": GFT_EXCERPT_RUNES is the only flag");
    return excerpt_run(e, kWhoPlain, d_text_blob, d_doc_off, n_docs, d_span_off, d_span_start, d_span_len, before, after, flags, 0, d_out, cap_bytes,
                       d_exc_off, d_exc_doc, d_exc_start, d_exc_span_off, cap_exc, d_span_rel, d_doc_exc_off, n_exc, total_bytes);
} GFT_CATCH((e ? &e->err : nullptr))

int gft_excerpt_spans_snap_device(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs,
                                  const uint64_t* d_span_off, const uint32_t* d_span_start, const uint32_t* d_span_len, uint32_t before,
                                  uint32_t after, uint32_t flags, uint32_t reach, uint8_t* d_out, uint64_t cap_bytes, uint64_t* d_exc_off,
                                  uint64_t* d_exc_doc, uint32_t* d_exc_start, uint64_t* d_exc_span_off, uint64_t cap_exc, uint32_t* d_span_rel,
                                  uint64_t* d_doc_exc_off, uint64_t* n_exc, uint64_t* total_bytes) try {
    if (!e) return GFT_E_INVALID;
    GFT_LOCK(e);
    if (n_exc) *n_exc = 0;
    if (total_bytes) *total_bytes = 0;
    if (flags & ~(uint32_t)(GFT_EXCERPT_RUNES | GFT_EXCERPT_WORDS | GFT_EXCERPT_LINES)) return fail(e, GFT_E_INVALID, std::string(kWhoSnap) + ": unknown flag bits");
    if ((flags & GFT_EXCERPT_WORDS) && (flags & GFT_EXCERPT_LINES))
        return fail(e, GFT_E_INVALID, std::string(kWhoSnap) + ": GFT_EXCERPT_WORDS and GFT_EXCERPT_LINES exclude each other");
    if (reach > GFT_EXCERPT_REACH_MAX) return fail(e, GFT_E_INVALID, std::string(kWhoSnap) + ": reach beyond GFT_EXCERPT_REACH_MAX");
    return excerpt_run(e, kWhoSnap, d_text_blob, d_doc_off, n_docs, d_span_off, d_span_start, d_span_len, before, after, flags, reach, d_out,
                       cap_bytes, d_exc_off, d_exc_doc, d_exc_start, d_exc_span_off, cap_exc, d_span_rel, d_doc_exc_off, n_exc, total_bytes);
} GFT_CATCH((e ? &e->err : nullptr))

int gft_debug_excerpt_spans(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const uint64_t* span_off,
                            const uint32_t* span_start, const uint32_t* span_len, uint32_t before, uint32_t after, uint32_t flags,
                            uint8_t* out, uint64_t cap_bytes, uint64_t* exc_off, uint64_t* exc_doc, uint32_t* exc_start,
                            uint64_t* exc_span_off, uint64_t cap_exc, uint32_t* span_rel, uint64_t* doc_exc_off, uint64_t* n_exc,
                            uint64_t* total_bytes) try {
    return excerpt_spans_host(blob, doc_off, n_docs, span_off, span_start, span_len, before, after, flags, out, cap_bytes, exc_off, exc_doc,
                              exc_start, exc_span_off, cap_exc, span_rel, doc_exc_off, n_exc, total_bytes);
} GFT_CATCH(nullptr)

int gft_debug_excerpt_spans_snap(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const uint64_t* span_off,
                                 const uint32_t* span_start, const uint32_t* span_len, uint32_t before, uint32_t after, uint32_t flags,
                                 uint32_t reach, uint8_t* out, uint64_t cap_bytes, uint64_t* exc_off, uint64_t* exc_doc, uint32_t* exc_start,
                                 uint64_t* exc_span_off, uint64_t cap_exc, uint32_t* span_rel, uint64_t* doc_exc_off, uint64_t* n_exc,
                                 uint64_t* total_bytes) try {
    return excerpt_spans_snap_host(blob, doc_off, n_docs, span_off, span_start, span_len, before, after, flags, reach, word_table_host(), out,
                                   cap_bytes, exc_off, exc_doc, exc_start, exc_span_off, cap_exc, span_rel, doc_exc_off, n_exc, total_bytes);
} GFT_CATCH(nullptr)

int gft_debug_excerpt_snap_edges(const uint8_t* doc, uint64_t L, uint64_t lo, uint64_t hi, uint32_t flags, uint32_t reach, uint64_t* lo_out,
                                 uint64_t* hi_out) try {
    if (!exc_snap_args_ok(flags, reach) || lo > hi || hi > L || (L && !doc)) return GFT_E_INVALID;
    exc_snap_window<true>(word_table_host(), doc, L, flags, reach, lo, hi);
    if (lo_out) *lo_out = lo;
    if (hi_out) *hi_out = hi;
    return GFT_OK;
} GFT_CATCH(nullptr)

void gft_debug_excerpt_shape(uint32_t* tile_spans, uint32_t* trip_tiles) {
    if (tile_spans) *tile_spans = kExcTile;
    if (trip_tiles) *trip_tiles = kExcCarryTiles;
}

}  // extern "C"
