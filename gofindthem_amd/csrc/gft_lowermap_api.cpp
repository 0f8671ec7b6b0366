// gft_lowermap_api.cpp -- spans of a lowered batch mapped back to the source text (gft_lowermap.hip): gft_map_spans_to_source_device,
// and the host walk behind gft_debug_map_spans_to_source.
#include "gft_engine.hpp"
#include "gft_lowermap.hpp"
#include "gft_overlap.hpp"

using namespace gft;
using namespace gft::api;

namespace {
constexpr RoomTexts kMapRoom{"no device memory for the span map's work buffers", "span map alloc"};
const char kWho[] = "gft_map_spans_to_source_device";

// a span array (the call rewrites entries [s0, s0 + n) of both in place) overlaps the text [lo, hi) of the blob, the offsets or the
// other span array
bool map_buffers_overlap(const uint8_t* text, uint64_t lo, uint64_t hi, const uint64_t* doc_off, uint64_t n_docs, const uint64_t* span_off,
                         const uint32_t* span_start, const uint32_t* span_len, uint64_t s0, uint64_t n) {
    const ByteRange outs[] = {{span_start + s0, n * 4}, {span_len + s0, n * 4}};
    const ByteRange ins[] = {{text ? text + lo : nullptr, hi > lo ? hi - lo : 0}, {doc_off, (n_docs + 1) * 8}, {span_off, (n_docs + 1) * 8}};
    return outputs_overlap(outs, ins);
}

int map_spans(gft_engine* e, const uint8_t* d_text, const uint64_t* d_doc_off, uint64_t n_docs, const uint64_t* d_span_off, uint32_t* d_span_start,
              uint32_t* d_span_len, uint64_t limit) {
    if (n_docs && (!d_doc_off || !d_span_off)) return fail(e, GFT_E_INVALID, "null argument");
    if (!e->peers.empty()) return fail(e, GFT_E_UNSUPPORTED, std::string(kWho) + ": single-device handles only");
    int rc = check_ready(e, kNeedDevice | kNeedSettled, kWho);
    if (rc) return rc;
    if (n_docs > (~0ull >> 4)) return fail(e, GFT_E_INVALID, std::string(kWho) + ": a size beyond the address space");
    if (!n_docs) return GFT_OK;
    DeviceGuard g(e->device);
    hipStream_t st = e->stream;
    uint64_t ends[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(&ends[0], d_span_off, 8, hipMemcpyDeviceToHost, st), "span offsets");
    HIP_TRY(hipMemcpyAsync(&ends[1], d_span_off + n_docs, 8, hipMemcpyDeviceToHost, st), "span offsets");
    HIP_TRY(hipStreamSynchronize(st), "span offsets");
    if (ends[1] < ends[0] || ends[1] - ends[0] > (~0ull >> 4)) return fail(e, GFT_E_INVALID, std::string(kWho) + ": span offsets descend");
    const uint64_t n = std::min(ends[1], std::max(limit, ends[0])) - ends[0];
    if (!n) return GFT_OK;
    if (!d_text || !d_span_start || !d_span_len) return fail(e, GFT_E_INVALID, "null argument");
    auto& M = e->d_lmap;
    if ((rc = room(e, M.off, (n_docs + 1) * 8, kMapRoom))) return rc;
    uint64_t nu = 0, total = 0, range[2] = {0, 0};
    if ((rc = lower_count(e, d_text, d_doc_off, n_docs, nullptr, 0, M.off.as<uint64_t>(), &nu, &total, kWho, "lowermap_table", range))) return rc;
    if (map_buffers_overlap(d_text, range[0], range[1], d_doc_off, n_docs, d_span_off, d_span_start, d_span_len, ends[0], n))
        return fail(e, GFT_E_INVALID, std::string(kWho) + ": a span array overlaps the text, the offsets or the other span array");
    const uint64_t slots = lowermap_slots(range[1] - range[0], nu);
    if ((rc = room(e, M.tab, slots * 4, kMapRoom)) || (rc = room(e, M.mapped, n * 8, kMapRoom)) || (rc = room(e, M.ctl, 4, kMapRoom))) return rc;
    const LowerTable T{e->d_lw.page.as<uint16_t>(), e->d_lw.delta.as<int32_t>(), (uint32_t)lower_table_host().page.size()};
    {
        ProfScope ps(e, "lowermap_table");
        HIP_TRY(launch_lower_table(d_text, d_doc_off, e->d_lw.units.as<Unit>(), nu, T, e->d_lw.unit_base.as<uint64_t>(), e->d_lw.unit_out.as<uint64_t>(),
                                   range[0], M.tab.as<uint32_t>(), e->n_cus, st), "span map table kernel launch");
    }
    LowerMapParams P{};
    P.V = LowerMapView{d_text, d_doc_off, n_docs, e->d_lw.unit_base.as<uint64_t>(), e->d_lw.units.as<Unit>(), e->d_lw.unit_out.as<uint64_t>(),
                       M.tab.as<uint32_t>(), T};
    P.span_off = d_span_off; P.span_start = d_span_start; P.span_len = d_span_len; P.s0 = ends[0]; P.n_spans = n;
    P.mapped = M.mapped.as<uint32_t>(); P.ctl = M.ctl.as<uint32_t>();
    {
        ProfScope ps(e, "lowermap_spans");
        HIP_TRY(hipMemsetAsync(P.ctl, 0, 4, st), "span map check");
        HIP_TRY(launch_lowermap_check(P, st), "span map check kernel launch");
        HIP_TRY(launch_lowermap_write(P, st), "span map write kernel launch");
    }
    uint32_t h_ctl = 0;
    HIP_TRY(hipMemcpyAsync(&h_ctl, P.ctl, 4, hipMemcpyDeviceToHost, st), "span map flag");
    HIP_TRY(hipStreamSynchronize(st), "span map write");
    if (h_ctl) return fail(e, GFT_E_INVALID, std::string(kWho) + ": a span reaches past the end of its document's lower-case form (nothing was written)");
    return GFT_OK;
}
}  // namespace

extern "C" {

int gft_map_spans_limit(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs, const uint64_t* d_span_off,
                        uint32_t* d_span_start, uint32_t* d_span_len, uint64_t limit) try {
    if (!e) return GFT_E_INVALID;
    GFT_LOCK(e);
    return map_spans(e, d_text_blob, d_doc_off, n_docs, d_span_off, d_span_start, d_span_len, limit);
} GFT_CATCH((e ? &e->err : nullptr))

int gft_map_spans_to_source_device(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs, const uint64_t* d_span_off,
                                   uint32_t* d_span_start, uint32_t* d_span_len) try {
    if (!e) return GFT_E_INVALID;
    GFT_LOCK(e);
    return map_spans(e, d_text_blob, d_doc_off, n_docs, d_span_off, d_span_start, d_span_len, ~0ull);
} GFT_CATCH((e ? &e->err : nullptr))

int gft_debug_map_spans_to_source(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const uint64_t* span_off, uint32_t* span_start,
                                  uint32_t* span_len) try {
    if (n_docs && (!doc_off || !span_off)) return GFT_E_INVALID;
    if (!n_docs) return GFT_OK;
    for (uint64_t d = 0; d < n_docs; d++)
        if (doc_off[d + 1] < doc_off[d] || doc_off[d + 1] - doc_off[d] > 0xFFFFFFFFull) return GFT_E_INVALID;
    if (doc_off[n_docs] > doc_off[0] && !blob) return GFT_E_INVALID;
    // (the pieces load up to 20 bytes from their first one: the walk runs on a copy with the slack the device entry asks of its
    // caller; offsets are rebased to it -- as gft_debug_emulate_to_lower.  The overlap check looks at the caller's buffers.)
    const uint64_t lo = doc_off[0], len = doc_off[n_docs] - lo;
    for (uint64_t d = 0; d < n_docs; d++)
        if (span_off[d + 1] < span_off[d]) return GFT_E_INVALID;
    const uint64_t s0 = span_off[0], n = span_off[n_docs] - s0;
    if (!n) return GFT_OK;
    if (!span_start || !span_len) return GFT_E_INVALID;
    if (map_buffers_overlap(blob, lo, lo + len, doc_off, n_docs, span_off, span_start, span_len, s0, n)) return GFT_E_INVALID;
    std::vector<uint8_t> text((size_t)len + 64, 0);
    if (len) memcpy(text.data(), blob + lo, (size_t)len);
    std::vector<uint64_t> off(n_docs + 1);
    for (uint64_t d = 0; d <= n_docs; d++) off[d] = doc_off[d] - lo;
    return lowermap_host(text.data(), off.data(), n_docs, span_off, span_start, span_len, ~0ull);
} GFT_CATCH(nullptr)

void gft_debug_lowermap_shape(uint32_t* piece_bytes, uint32_t* trip_bytes, uint32_t* unit_bytes, uint32_t* tile_spans) {
    if (piece_bytes) *piece_bytes = kLowerPiece;
    if (trip_bytes) *trip_bytes = kLowerChunk;
    if (unit_bytes) *unit_bytes = kLowerUnitMax;
    if (tile_spans) *tile_spans = kMapTile;
}

}  // extern "C"
