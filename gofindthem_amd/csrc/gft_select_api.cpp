// gft_select_api.cpp -- the documents that matched, gathered into one blob (gft_select.hip): gft_select_docs_device, and the host
// walk behind gft_debug_select_docs.
#include "gft_doc_gather.hpp"

using namespace gft;
using namespace gft::api;

namespace {
constexpr DocGather kSelect{"gft_select_docs_device", "select", {"no device memory for the select's work buffers", "select alloc"}};
}

extern "C" {

int gft_select_docs_device(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs, const uint32_t* d_bitmap,
                           uint32_t n_cols, const uint32_t* want, uint32_t mode, const uint8_t* d_also, uint8_t* d_out, uint64_t cap_bytes,
                           uint64_t* d_out_off, uint64_t* d_doc_idx, uint64_t cap_docs, uint64_t* n_selected, uint64_t* total_bytes) try {
    if (!e) return GFT_E_INVALID;
    GFT_LOCK(e);
    if (n_selected) *n_selected = 0;
    if (total_bytes) *total_bytes = 0;
    const uint32_t W = (n_cols + 31) / 32;
    if (n_docs && (!d_doc_off || !d_text_blob || (W && !d_bitmap))) return fail(e, GFT_E_INVALID, "null argument");
    if (cap_bytes && !d_out) return fail(e, GFT_E_INVALID, "gft_select_docs_device: cap_bytes but no output buffer");
    if (cap_docs && (!d_out_off || !d_doc_idx)) return fail(e, GFT_E_INVALID, "gft_select_docs_device: cap_docs but no offset or index array");
    if (!e->peers.empty()) return fail(e, GFT_E_UNSUPPORTED, "gft_select_docs_device: single-device handles only");
    int rc = check_ready(e, kNeedDevice | kNeedSettled, "gft_select_docs_device");
    if (rc) return rc;
    if (mode != GFT_SELECT_ANY && mode != GFT_SELECT_ALL && mode != GFT_SELECT_NONE) return fail(e, GFT_E_INVALID, "gft_select_docs_device: unknown mode");
    if (cap_docs > (~0ull >> 4) || n_docs > (~0ull >> 4)) return fail(e, GFT_E_INVALID, "gft_select_docs_device: a size beyond the address space");
    DeviceGuard g(e->device);
    hipStream_t st = e->stream;
    if (!n_docs) return doc_gather_empty(e, kSelect, d_out_off);
    auto& S = e->d_select;
    std::vector<uint32_t> h_want(std::max<uint32_t>(W, 1), 0);
    SyncOnExit drain(e);                                            // (h_want is handed to an asynchronous copy)
    select_want_words(want, n_cols, h_want.data());
    if ((rc = room(e, S.want, (uint64_t)W * 4, kSelect.room)) || (rc = room(e, S.len, n_docs * 4, kSelect.room)) ||
        (rc = room(e, S.sel, n_docs * 4, kSelect.room)) || (rc = room(e, S.pos, (n_docs + 1) * 8, kSelect.room)) ||
        (rc = room(e, S.rank, (n_docs + 1) * 8, kSelect.room)) || (rc = room(e, S.partial, scan_partials_needed(n_docs) * 8, kSelect.room)) ||
        (rc = room(e, S.ctl, kSelCtlWords * 8, kSelect.room)))
        return rc;
    SelectParams P{};
    P.pos = S.pos.as<uint64_t>(); P.rank = S.rank.as<uint64_t>();
    if ((rc = doc_gather_select_mark(e, kSelect, P, d_text_blob, d_doc_off, n_docs, d_bitmap, n_cols, mode, d_also, h_want.data(), S.want, S.len, S.sel,
                                     S.ctl, kSelCtlWords)))
        return rc;
    {
        ProfScope ps(e, "select_scan");
        HIP_TRY(launch_exclusive_scan(P.len, n_docs, S.pos.as<uint64_t>(), S.partial.as<uint64_t>(), st), "select scan");
        HIP_TRY(launch_exclusive_scan(P.sel, n_docs, S.rank.as<uint64_t>(), S.partial.as<uint64_t>(), st), "select scan");
        HIP_TRY(launch_select_pack(P, st), "select scan");
    }
    uint64_t h_ctl[kSelCtlWords] = {0};
    if ((rc = doc_gather_read(e, kSelect, P.ctl, h_ctl, kSelCtlWords))) return rc;
    if (select_buffers_overlap(d_text_blob, h_ctl[kSelCtlLo], h_ctl[kSelCtlHi], d_doc_off, n_docs, d_bitmap, n_cols, d_also, d_out, cap_bytes,
                               d_out_off, d_doc_idx, cap_docs))
        return doc_gather_overlap(e, kSelect);
    P.total = h_ctl[kSelCtlTotal]; P.m = h_ctl[kSelCtlM];
    if (n_selected) *n_selected = P.m;
    if (total_bytes) *total_bytes = P.total;
    if ((rc = room(e, S.c_off, (P.m + 1) * 8, kSelect.room)) || (rc = room(e, S.c_src, P.m * 8, kSelect.room))) return rc;
    P.c_off = S.c_off.as<uint64_t>(); P.c_src = S.c_src.as<uint64_t>();
    P.out_off = d_out_off; P.doc_idx = d_doc_idx; P.cap_docs = cap_docs;
    {
        ProfScope ps(e, "select_place");
        HIP_TRY(launch_select_place(P, st), "select place kernel launch");
    }
    return doc_gather_copy(e, kSelect, d_text_blob, P.c_off, P.c_src, P.m, P.total, d_out, cap_bytes);
} GFT_CATCH((e ? &e->err : nullptr))

int gft_debug_select_docs(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const uint32_t* bitmap, uint32_t n_cols,
                          const uint32_t* want, uint32_t mode, const uint8_t* also, uint8_t* out, uint64_t cap_bytes, uint64_t* out_off,
                          uint64_t* doc_idx, uint64_t cap_docs, uint64_t* n_selected, uint64_t* total_bytes) try {
    return select_docs_host(blob, doc_off, n_docs, bitmap, n_cols, want, mode, also, out, cap_bytes, out_off, doc_idx, cap_docs, n_selected,
                            total_bytes);
} GFT_CATCH(nullptr)

void gft_debug_select_shape(uint32_t* chunk_bytes, uint32_t* trip_bytes, uint32_t* tile_bytes) {
    if (chunk_bytes) *chunk_bytes = kSelChunk;
    if (trip_bytes) *trip_bytes = kSelTrip;
    if (tile_bytes) *tile_bytes = kSelTile;
}

}  // extern "C"
