// gft_route_api.cpp -- documents routed to per-bucket runs of one blob (gft_route.hip): gft_route_docs_device, and the host walk
// behind gft_debug_route_docs.
#include "gft_doc_gather.hpp"
#include "gft_route.hpp"

using namespace gft;
using namespace gft::api;

namespace {
constexpr DocGather kRoute{"gft_route_docs_device", "route", {"no device memory for the route's work buffers", "route alloc"}};
#define GFT_STR2(x) #x
#define GFT_STR(x) GFT_STR2(x)
}

extern "C" {

int gft_route_docs_device(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs, const uint32_t* d_bitmap,
                          uint32_t n_cols, const uint32_t* masks, uint32_t n_buckets, uint32_t mode, uint32_t flags, const uint8_t* d_also,
                          uint8_t* d_out, uint64_t cap_bytes, uint64_t* d_out_off, uint64_t* d_doc_idx, uint64_t cap_docs, uint64_t* bucket_doc,
                          uint64_t* bucket_byte) try {
    if (!e) return GFT_E_INVALID;
    GFT_LOCK(e);
    if (flags & ~GFT_ROUTE_REST) return fail(e, GFT_E_INVALID, "gft_route_docs_device: unknown flag bits");
    const uint32_t rest = (flags & GFT_ROUTE_REST) ? 1u : 0u;
    if (n_buckets > GFT_ROUTE_MAX_BUCKETS - rest)
        return fail(e, GFT_E_UNSUPPORTED, "gft_route_docs_device: more than " GFT_STR(GFT_ROUTE_MAX_BUCKETS) " buckets (GFT_ROUTE_MAX_BUCKETS), the rest bucket included");
    const uint32_t B = n_buckets + rest, W = (n_cols + 31) / 32;
    for (uint32_t b = 0; b <= B; b++) {
        if (bucket_doc) bucket_doc[b] = 0;
        if (bucket_byte) bucket_byte[b] = 0;
    }
    if (n_docs && (!d_doc_off || !d_text_blob || (W && !d_bitmap))) return fail(e, GFT_E_INVALID, "null argument");
    if (n_buckets && W && !masks) return fail(e, GFT_E_INVALID, "gft_route_docs_device: buckets but no masks");
    if (cap_bytes && !d_out) return fail(e, GFT_E_INVALID, "gft_route_docs_device: cap_bytes but no output buffer");
    if (cap_docs && (!d_out_off || !d_doc_idx)) return fail(e, GFT_E_INVALID, "gft_route_docs_device: cap_docs but no offset or index array");
    if (!e->peers.empty()) return fail(e, GFT_E_UNSUPPORTED, "gft_route_docs_device: single-device handles only");
    int rc = check_ready(e, kNeedDevice | kNeedSettled, "gft_route_docs_device");
    if (rc) return rc;
    if (mode != GFT_ROUTE_FIRST && mode != GFT_ROUTE_EVERY) return fail(e, GFT_E_INVALID, "gft_route_docs_device: unknown mode");
    if (d_also && !rest) return fail(e, GFT_E_INVALID, "gft_route_docs_device: d_also needs GFT_ROUTE_REST");
    if (cap_docs > (~0ull >> 4) || n_docs > (~0ull >> 4)) return fail(e, GFT_E_INVALID, "gft_route_docs_device: a size beyond the address space");
    DeviceGuard g(e->device);
    hipStream_t st = e->stream;
    if (!n_docs) return doc_gather_empty(e, kRoute, d_out_off);
    auto& S = e->d_route;
    const uint64_t n_tiles = route_tiles(n_docs), n_cells = (uint64_t)B * n_tiles;
    std::vector<uint32_t> h_masks(std::max<uint64_t>((uint64_t)n_buckets * W, 1), 0);
    SyncOnExit drain(e);                                            // (h_masks is handed to an asynchronous copy)
    if (W) route_mask_words(masks, n_buckets, n_cols, h_masks.data());
    if ((rc = room(e, S.masks, (uint64_t)n_buckets * W * 4, kRoute.room)) || (rc = room(e, S.member, n_docs * 8, kRoute.room)) ||
        (rc = room(e, S.len, n_docs * 4, kRoute.room)) || (rc = room(e, S.cnt, n_cells * 4, kRoute.room)) ||
        (rc = room(e, S.tile_bytes, n_tiles * 8, kRoute.room)) || (rc = room(e, S.base, (n_cells + 1) * 8, kRoute.room)) ||
        (rc = room(e, S.partial, scan_partials_needed(n_cells) * 8, kRoute.room)) || (rc = room(e, S.ctl, kRouteCtlWords * 8, kRoute.room)))
        return rc;
    RouteParams P{};
    P.doc_off = d_doc_off; P.n_docs = n_docs; P.n_tiles = n_tiles; P.bitmap = d_bitmap;
    P.W = W; P.lg = bit_row_lg(W);
    P.n_buckets = n_buckets; P.B = B; P.mode = mode; P.rest = rest; P.masks = S.masks.as<uint32_t>(); P.also = d_also;
    P.member = S.member.as<uint64_t>(); P.len = S.len.as<uint32_t>(); P.cnt = S.cnt.as<uint32_t>(); P.tile_bytes = S.tile_bytes.as<uint64_t>();
    P.base = S.base.as<uint64_t>(); P.ctl = S.ctl.as<uint64_t>();
    {
        ProfScope ps(e, "route_mark");
        if (n_buckets && W)
            HIP_TRY(hipMemcpyAsync(S.masks.p, h_masks.data(), (size_t)n_buckets * W * 4, hipMemcpyHostToDevice, st), "route mask upload");
        HIP_TRY(hipMemsetAsync(P.ctl, 0, kRouteCtlWords * 8, st), "route mark");
        HIP_TRY(launch_route_mark(P, e->n_cus, st), "route mark kernel launch");
    }
    {
        ProfScope ps(e, "route_count");
        HIP_TRY(launch_route_count(P, e->n_cus, st), "route count kernel launch");
    }
    {
        ProfScope ps(e, "route_scan");
        HIP_TRY(launch_exclusive_scan(P.cnt, n_cells, S.base.as<uint64_t>(), S.partial.as<uint64_t>(), st), "route scan");
        HIP_TRY(launch_route_pack(P, st), "route scan");
    }
    uint64_t h_ctl[kRouteCtlWords] = {0};
    if ((rc = doc_gather_read(e, kRoute, P.ctl, h_ctl, kRouteCtlDoc + B + 1))) return rc;
    if (route_buffers_overlap(d_text_blob, h_ctl[kRouteCtlLo], h_ctl[kRouteCtlHi], d_doc_off, n_docs, d_bitmap, n_cols, masks, n_buckets, d_also, d_out,
                              cap_bytes, d_out_off, d_doc_idx, cap_docs, bucket_doc, bucket_byte, B))
        return doc_gather_overlap(e, kRoute);
    P.m = h_ctl[kRouteCtlM];
    const uint64_t total = h_ctl[kRouteCtlTotal];
    if (bucket_doc)
        for (uint32_t b = 0; b <= B; b++) bucket_doc[b] = h_ctl[kRouteCtlDoc + b];
    if (!bucket_byte && !d_out_off && !cap_bytes && !cap_docs) return GFT_OK;      // a count of documents: the answer is here
    if ((rc = room(e, S.ent_len, P.m * 4, kRoute.room)) || (rc = room(e, S.c_off, (P.m + 1) * 8, kRoute.room)) ||
        (rc = room(e, S.c_src, P.m * 8, kRoute.room)) || (rc = room(e, S.partial, scan_partials_needed(std::max(P.m, n_cells)) * 8, kRoute.room)))
        return rc;
    P.ent_len = S.ent_len.as<uint32_t>(); P.c_src = S.c_src.as<uint64_t>(); P.c_off = S.c_off.as<uint64_t>();
    P.out_off = d_out_off; P.doc_idx = d_doc_idx; P.cap_docs = cap_docs;
    {
        ProfScope ps(e, "route_place");
        HIP_TRY(launch_route_place(P, e->n_cus, st), "route place kernel launch");
    }
    {
        ProfScope ps(e, "route_scan");
        HIP_TRY(launch_exclusive_scan(P.ent_len, P.m, S.c_off.as<uint64_t>(), S.partial.as<uint64_t>(), st), "route scan");
        HIP_TRY(launch_route_finish(P, st), "route scan");
    }
    if ((rc = select_copy_run(e, d_text_blob, P.c_off, P.c_src, P.m, total, d_out, cap_bytes, "route_copy", "route copy kernel launch"))) return rc;
    HIP_TRY(hipMemcpyAsync(h_ctl + kRouteCtlByte, P.ctl + kRouteCtlByte, (B + 1) * 8, hipMemcpyDeviceToHost, st), "route copy");
    HIP_TRY(hipStreamSynchronize(st), "route copy");
    if (bucket_byte)
        for (uint32_t b = 0; b <= B; b++) bucket_byte[b] = h_ctl[kRouteCtlByte + b];
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

int gft_debug_route_docs(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const uint32_t* bitmap, uint32_t n_cols,
                         const uint32_t* masks, uint32_t n_buckets, uint32_t mode, uint32_t flags, const uint8_t* also, uint8_t* out,
                         uint64_t cap_bytes, uint64_t* out_off, uint64_t* doc_idx, uint64_t cap_docs, uint64_t* bucket_doc, uint64_t* bucket_byte) try {
    return route_docs_host(blob, doc_off, n_docs, bitmap, n_cols, masks, n_buckets, mode, flags, also, out, cap_bytes, out_off, doc_idx, cap_docs,
                           bucket_doc, bucket_byte);
} GFT_CATCH(nullptr)

void gft_debug_route_shape(uint32_t* tile_docs) {
    if (tile_docs) *tile_docs = kRouteTileDocs;
}

}  // extern "C"
