// gft_mark_api.cpp -- highlight: markers written round the hit spans (gft_mark.hip, the run passes of gft_excerpt.hip):
// gft_mark_spans_device, and the host walk behind gft_debug_mark_spans.
#include <string.h>

#include "gft_engine.hpp"
#include "gft_mark.hpp"
#include "gft_span_runs.hpp"

using namespace gft;
using namespace gft::api;

namespace {
constexpr RoomTexts kMarkRoom{"no device memory for the highlight's work buffers", "mark alloc"};
const char kWho[] = "gft_mark_spans_device";
}  // namespace

extern "C" {

int gft_mark_spans_device(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs,
                          const uint64_t* d_span_off, const uint32_t* d_span_start, const uint32_t* d_span_len, const uint8_t* open,
                          uint32_t open_len, const uint8_t* close, uint32_t close_len, uint32_t flags, uint8_t* d_out, uint64_t cap_bytes,
                          uint64_t* d_out_off, uint32_t* d_span_new, uint64_t* d_doc_run_off, uint64_t* n_runs, uint64_t* total_bytes) try {
    if (!e) return GFT_E_INVALID;
    GFT_LOCK(e);
    if (n_runs) *n_runs = 0;
    if (total_bytes) *total_bytes = 0;
    if (flags) return fail(e, GFT_E_INVALID, std::string(kWho) + ": flags must be 0");
    if (open_len > GFT_MARK_MAX || close_len > GFT_MARK_MAX)
        return fail(e, GFT_E_INVALID, std::string(kWho) + ": a marker has GFT_MARK_MAX bytes at most");
    if ((open_len && !open) || (close_len && !close)) return fail(e, GFT_E_INVALID, std::string(kWho) + ": a marker length but no marker");
    if (n_docs && (!d_doc_off || !d_span_off)) return fail(e, GFT_E_INVALID, "null argument");
    if (cap_bytes && !d_out) return fail(e, GFT_E_INVALID, std::string(kWho) + ": cap_bytes but no output buffer");
    if (!e->peers.empty()) return fail(e, GFT_E_UNSUPPORTED, std::string(kWho) + ": single-device handles only");
    int rc = check_ready(e, kNeedDevice | kNeedSettled, kWho);
    if (rc) return rc;
    if (n_docs > (~0ull >> 4)) return fail(e, GFT_E_INVALID, std::string(kWho) + ": a size beyond the address space");
    DeviceGuard g(e->device);
    hipStream_t st = e->stream;
    uint8_t block[kMarkWords * 8];                                  // the markers, copied out of the caller's memory (outlives the drain)
    // the run passes are the excerpt's, in the excerpt's buffers (gft_span_runs.hpp)
    auto& X = e->d_excerpt;
    auto& K = e->d_mark;
    SyncOnExit drain(e);                                            // (the pinned words are handed to asynchronous copies)
    MarkParams P{};
    P.X.V = ExcView{d_text_blob, d_doc_off, n_docs, d_span_off, d_span_start, d_span_len, 0, 0, 0};
    SpanRun R{kWho, "mark", "heads", kMarkRoom};
    if ((rc = span_run_begin(e, P.X, R))) return rc;
    const uint64_t n = R.n;
    if (mark_buffers_overlap(d_text_blob, R.lo, R.hi, d_doc_off, n_docs, d_span_off, d_span_start, d_span_len, R.s0, n, d_out, cap_bytes, d_out_off,
                             d_span_new, d_doc_run_off))
        return fail(e, GFT_E_INVALID, std::string(kWho) + ": an output overlaps an input or another output");
    if ((rc = span_run_room(e, P.X, R, false)) || (rc = room(e, K.marks, kMarkWords * 8, kMarkRoom))) return rc;
    P.M = MarkPlan{nullptr, 0, R.lo, R.hi - R.lo, open_len, close_len};
    if ((rc = span_run_launch(e, P.X, R, "mark_runs", "mark_runs"))) return rc;
    {
        ProfScope ps(e, "mark_scan");
        if (n) {
            HIP_TRY(launch_exclusive_scan(P.X.head, n, X.rank.as<uint64_t>(), X.partial.as<uint64_t>(), st), "mark scan");
        } else {
            HIP_TRY(hipMemsetAsync(X.rank.p, 0, 8, st), "mark scan");   // (no span: rank[0] is what the passes behind read)
        }
        HIP_TRY(launch_mark_check(P, st), "mark check kernel launch");
    }
    const uint64_t* h_ctl = X.pin;
    HIP_TRY(hipMemcpyAsync(X.pin, P.X.ctl, (kMarkCtlGrow + 1) * 8, hipMemcpyDeviceToHost, st), "mark totals");
    HIP_TRY(hipStreamSynchronize(st), "mark totals");
    if ((rc = span_run_verdict(e, R, h_ctl))) return rc;
    if (h_ctl[kMarkCtlGrow])
        return fail(e, GFT_E_INVALID, std::string(kWho) + ": a document would reach 4 GiB once marked (nothing was written)");
    const uint64_t runs = h_ctl[kExcCtlExc], total = (R.hi - R.lo) + runs * ((uint64_t)open_len + close_len);
    if (n_runs) *n_runs = runs;
    if (total_bytes) *total_bytes = total;
    if ((rc = room(e, K.q, 2 * runs * 8, kMarkRoom))) return rc;
    P.q = K.q.as<uint64_t>();
    P.M.q = P.q; P.M.nq = 2 * runs;
    P.marks = K.marks.as<uint64_t>();
    P.out_off = d_out_off; P.span_new = d_span_new; P.doc_run_off = d_doc_run_off;
    P.out = d_out;
    P.G = sel_geom(total, cap_bytes, d_out);
    {
        ProfScope ps(e, "mark_place");
        HIP_TRY(launch_mark_place(P, st), "mark place kernel launch");
        if (!n_docs && d_out_off) HIP_TRY(hipMemsetAsync(d_out_off, 0, 8, st), "mark offsets");
        if (!n_docs && d_doc_run_off) HIP_TRY(hipMemsetAsync(d_doc_run_off, 0, 8, st), "mark offsets");
    }
    if (P.G.end) {
        // the markers are the caller's host memory: into a block of this call's own, then onto the device
        memset(block, 0, sizeof block);
        if (open_len) memcpy(block, open, open_len);
        if (close_len) memcpy(block + kMarkSlot, close, close_len);
        HIP_TRY(hipMemcpyAsync(K.marks.p, block, sizeof block, hipMemcpyHostToDevice, st), "mark markers");
        ProfScope ps(e, "mark_copy");
        HIP_TRY(launch_mark_copy(P, st), "mark copy kernel launch");
    }
    HIP_TRY(hipStreamSynchronize(st), "mark copy");
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

int gft_debug_mark_spans(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const uint64_t* span_off, const uint32_t* span_start,
                         const uint32_t* span_len, const uint8_t* open, uint32_t open_len, const uint8_t* close, uint32_t close_len,
                         uint32_t flags, uint8_t* out, uint64_t cap_bytes, uint64_t* out_off, uint32_t* span_new, uint64_t* doc_run_off,
                         uint64_t* n_runs, uint64_t* total_bytes) try {
    return mark_spans_host(blob, doc_off, n_docs, span_off, span_start, span_len, open, open_len, close, close_len, flags, out, cap_bytes, out_off,
                           span_new, doc_run_off, n_runs, total_bytes);
} GFT_CATCH(nullptr)

void gft_debug_mark_shape(uint32_t* tile_spans, uint32_t* trip_tiles, uint32_t* chunk_bytes, uint32_t* tile_bytes) {
    if (tile_spans) *tile_spans = kExcTile;
    if (trip_tiles) *trip_tiles = kExcCarryTiles;
    if (chunk_bytes) *chunk_bytes = kSelChunk;
    if (tile_bytes) *tile_bytes = kSelTile;
}

}  // extern "C"
