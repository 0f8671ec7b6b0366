// gft_mark_api.cpp -- highlight: markers written round the hit spans (gft_mark.hip, the run passes of gft_excerpt.hip):
// gft_mark_spans_device, and the host walk behind gft_debug_mark_spans.
#include <string.h>

#include "gft_engine.hpp"
#include "gft_mark.hpp"

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
    // the run passes are the excerpt's, in the excerpt's buffers: the control block, its pinned landing place, the ends
    auto& X = e->d_excerpt;
    auto& K = e->d_mark;
    if ((rc = room(e, X.ctl, kExcCtlWords * 8, kMarkRoom))) return rc;
    if (!X.pin) HIP_TRY(hipHostMalloc((void**)&X.pin, kExcCtlWords * 8, hipHostMallocDefault), "pinned alloc");
    SyncOnExit drain(e);                                            // (the pinned words are handed to asynchronous copies)
    MarkParams P{};
    P.X.V = ExcView{d_text_blob, d_doc_off, n_docs, d_span_off, d_span_start, d_span_len, 0, 0, 0};
    P.X.ctl = X.ctl.as<uint64_t>();
    HIP_TRY(hipMemsetAsync(P.X.ctl, 0, kExcCtlWords * 8, st), "mark control block");
    uint64_t ends[4] = {0, 0, 0, 0};
    if (n_docs) {
        HIP_TRY(launch_excerpt_ends(P.X, st), "mark ends kernel launch");
        HIP_TRY(hipMemcpyAsync(X.pin, P.X.ctl + kExcCtlEnds, 32, hipMemcpyDeviceToHost, st), "span offsets");
        HIP_TRY(hipStreamSynchronize(st), "span offsets");
        for (int k = 0; k < 4; k++) ends[k] = X.pin[k];
    }
    if (ends[1] < ends[0] || ends[1] - ends[0] > (~0ull >> 4)) return fail(e, GFT_E_INVALID, std::string(kWho) + ": span offsets descend");
    if (ends[3] < ends[2]) return fail(e, GFT_E_INVALID, std::string(kWho) + ": document offsets descend, or a document of 4 GiB or more");
    const uint64_t s0 = ends[0], n = ends[1] - ends[0];
    if (n && (!d_span_start || !d_span_len)) return fail(e, GFT_E_INVALID, "null argument");
    if (ends[3] > ends[2] && !d_text_blob) return fail(e, GFT_E_INVALID, "null argument");
    if (mark_buffers_overlap(d_text_blob, ends[2], ends[3], d_doc_off, n_docs, d_span_off, d_span_start, d_span_len, s0, n, d_out, cap_bytes,
                             d_out_off, d_span_new, d_doc_run_off))
        return fail(e, GFT_E_INVALID, std::string(kWho) + ": an output overlaps an input or another output");
    const uint64_t n_tiles = exc_tiles(n);
    if ((rc = room(e, X.ws, n * 8, kMarkRoom)) || (rc = room(e, X.we, n * 8, kMarkRoom)) || (rc = room(e, X.sdoc, n * 8, kMarkRoom)) ||
        (rc = room(e, X.smin, n * 8, kMarkRoom)) || (rc = room(e, X.head, n * 4, kMarkRoom)) || (rc = room(e, X.share, n * 4, kMarkRoom)) ||
        (rc = room(e, X.rank, (n + 1) * 8, kMarkRoom)) || (rc = room(e, X.tmin, n_tiles * 8, kMarkRoom)) ||
        (rc = room(e, X.carry, n_tiles * 8, kMarkRoom)) ||
        (rc = room(e, X.partial, scan_partials_needed(std::max<uint64_t>(n, 1)) * 8, kMarkRoom)) ||
        (rc = room(e, K.marks, kMarkWords * 8, kMarkRoom)))
        return rc;
    P.X.s0 = s0; P.X.n_spans = n;
    P.X.ws = X.ws.as<uint64_t>(); P.X.we = X.we.as<uint64_t>(); P.X.sdoc = X.sdoc.as<uint64_t>(); P.X.smin = X.smin.as<uint64_t>();
    P.X.tmin = X.tmin.as<uint64_t>(); P.X.carry = X.carry.as<uint64_t>(); P.X.head = X.head.as<uint32_t>(); P.X.share = X.share.as<uint32_t>();
    P.X.rank = X.rank.as<uint64_t>();
    P.M = MarkPlan{nullptr, 0, ends[2], ends[3] - ends[2], open_len, close_len};
    {
        ProfScope ps(e, "mark_runs");
        HIP_TRY(launch_excerpt_docs(P.X, st), "mark document kernel launch");
        HIP_TRY(launch_excerpt_window(P.X, st), "mark window kernel launch");
        HIP_TRY(launch_excerpt_carry(P.X, st), "mark carry kernel launch");
        HIP_TRY(launch_excerpt_mark(P.X, st), "mark heads kernel launch");
    }
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
    if (h_ctl[kExcCtlOffs]) return fail(e, GFT_E_INVALID, std::string(kWho) + ": span offsets descend");
    if (h_ctl[kExcCtlDocs]) return fail(e, GFT_E_INVALID, std::string(kWho) + ": document offsets descend, or a document of 4 GiB or more");
    if (h_ctl[kExcCtlSpans])
        return fail(e, GFT_E_INVALID, std::string(kWho) + ": a span reaches past the end of its document, or the spans' ends descend inside a "
                                                          "document (nothing was written)");
    if (h_ctl[kMarkCtlGrow])
        return fail(e, GFT_E_INVALID, std::string(kWho) + ": a document would reach 4 GiB once marked (nothing was written)");
    const uint64_t runs = h_ctl[kExcCtlExc], total = (ends[3] - ends[2]) + runs * ((uint64_t)open_len + close_len);
    if (n_runs) *n_runs = runs;
    if (total_bytes) *total_bytes = total;
    if ((rc = room(e, K.q, 2 * runs * 8, kMarkRoom))) return rc;
    P.q = K.q.as<uint64_t>();
    P.M.q = P.q; P.M.nq = 2 * runs;
    P.marks = K.marks.as<uint64_t>();
    P.out_off = d_out_off; P.span_new = d_span_new; P.doc_run_off = d_doc_run_off;
    P.out = d_out;
    P.G = SelGeom{std::min(total, cap_bytes), (uint32_t)((uintptr_t)d_out & 15u)};
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
