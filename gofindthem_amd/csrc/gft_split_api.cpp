// gft_split_api.cpp -- a resident blob cut into line documents (gft_split.hip): gft_split_lines_device, and the host walk behind
// gft_debug_split_lines.
#include "gft_engine.hpp"
#include "gft_split.hpp"

using namespace gft;
using namespace gft::api;

namespace {
constexpr RoomTexts kSplitRoom{"no device memory for the split's work buffers", "split alloc"};
}

extern "C" {

int gft_split_lines_device(gft_engine* e, const uint8_t* d_blob, uint64_t len, uint32_t mode, uint64_t* d_doc_off, uint64_t cap,
                           uint64_t* n_docs) try {
    if (!e || !n_docs || (len && !d_blob)) return e ? fail(e, GFT_E_INVALID, "null argument") : GFT_E_INVALID;
    GFT_LOCK(e);
    *n_docs = 0;
    if (cap && !d_doc_off) return fail(e, GFT_E_INVALID, "gft_split_lines_device: cap entries but no output buffer");
    if (!e->peers.empty()) return fail(e, GFT_E_UNSUPPORTED, "gft_split_lines_device: single-device handles only");
    int rc = check_ready(e, kNeedDevice | kNeedSettled, "gft_split_lines_device");
    if (rc) return rc;
    if (mode != GFT_SPLIT_AFTER_NL && mode != GFT_SPLIT_JSON_LINES) return fail(e, GFT_E_INVALID, "gft_split_lines_device: unknown mode");
    if (cap > (~0ull >> 3) || len > ~0ull - 64) return fail(e, GFT_E_INVALID, "gft_split_lines_device: a size beyond the address space");
    if (cap) {
        const uintptr_t in = (uintptr_t)d_blob, out = (uintptr_t)d_doc_off;
        if (in < out + cap * 8 && out < in + len + 64) return fail(e, GFT_E_INVALID, "gft_split_lines_device: the output overlaps the input");
    }
    DeviceGuard g(e->device);
    hipStream_t st = e->stream;
    if (!len) {
        if (cap) HIP_TRY(hipMemsetAsync(d_doc_off, 0, 8, st), "split offsets");
        HIP_TRY(hipStreamSynchronize(st), "split offsets");
        return GFT_OK;
    }
    auto& S = e->d_split;
    SplitParams P{};
    P.blob = d_blob; P.len = len; P.n_tiles = split_tiles(len);
    if ((rc = room(e, S.cnt, P.n_tiles * 4, kSplitRoom)) || (rc = room(e, S.base, (P.n_tiles + 1) * 8, kSplitRoom)) ||
        (rc = room(e, S.partial, scan_partials_needed(P.n_tiles) * 8, kSplitRoom)))
        return rc;
    if (mode == GFT_SPLIT_JSON_LINES &&
        ((rc = room(e, S.sums, P.n_tiles * sizeof(SplitSum), kSplitRoom)) || (rc = room(e, S.carry, P.n_tiles * sizeof(SplitCarry), kSplitRoom))))
        return rc;
    P.sums = S.sums.as<SplitSum>(); P.carry = S.carry.as<SplitCarry>(); P.cnt = S.cnt.as<uint32_t>(); P.base = S.base.as<uint64_t>();
    P.out = d_doc_off; P.cap = cap;
    {
        ProfScope ps(e, "split_count");
        HIP_TRY(launch_split_count(P, mode, st), "split count kernel launch");
    }
    {
        ProfScope ps(e, "split_scan");
        if (mode == GFT_SPLIT_JSON_LINES) HIP_TRY(launch_split_carry(P, st), "split carry kernel launch");
        HIP_TRY(launch_exclusive_scan(P.cnt, P.n_tiles, S.base.as<uint64_t>(), S.partial.as<uint64_t>(), st), "split scan");
    }
    uint64_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, P.base + P.n_tiles, 8, hipMemcpyDeviceToHost, st), "split total");
    HIP_TRY(hipStreamSynchronize(st), "split count");
    *n_docs = total + (mode == GFT_SPLIT_AFTER_NL ? 1u : 0u);
    if (cap) {
        ProfScope ps(e, "split_write");
        HIP_TRY(launch_split_write(P, mode, st), "split write kernel launch");
    }
    HIP_TRY(hipStreamSynchronize(st), "split write");
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

int gft_debug_split_lines(const uint8_t* blob, uint64_t len, uint32_t mode, uint64_t* doc_off, uint64_t cap, uint64_t* n_docs) try {
    if (cap && doc_off && len) {
        const uintptr_t in = (uintptr_t)blob, out = (uintptr_t)doc_off;
        if (in < out + cap * 8 && out < in + len) return GFT_E_INVALID;
    }
    return split_lines_host(blob, len, mode, doc_off, cap, n_docs);
} GFT_CATCH(nullptr)

void gft_debug_split_shape(uint32_t* tile_bytes, uint32_t* tiles_per_carry_trip) {
    if (tile_bytes) *tile_bytes = kSplitTile;
    if (tiles_per_carry_trip) *tiles_per_carry_trip = kSplitCarryTrip;
}

}  // extern "C"
