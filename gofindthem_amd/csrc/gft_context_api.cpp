// gft_context_api.cpp -- context lines round the documents that matched (gft_context.hip): gft_context_docs_device, and the host
// walk behind gft_debug_context_docs.
#include "gft_context.hpp"
#include "gft_doc_gather.hpp"

using namespace gft;
using namespace gft::api;

namespace {
constexpr DocGather kContext{"gft_context_docs_device", "context", {"no device memory for the context call's work buffers", "context alloc"}};
}

extern "C" {

int gft_context_docs_device(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs, const uint32_t* d_bitmap,
                            uint32_t n_cols, const uint32_t* want, uint32_t mode, const uint8_t* d_also, uint64_t before, uint64_t after,
                            const uint8_t* d_fence, uint8_t* d_out, uint64_t cap_bytes, uint64_t* d_out_off, uint64_t* d_doc_idx, uint8_t* d_kind,
                            uint64_t cap_docs, uint64_t* d_group_off, uint64_t cap_groups, uint64_t* n_kept, uint64_t* n_hits, uint64_t* n_groups,
                            uint64_t* total_bytes) try {
    if (!e) return GFT_E_INVALID;
    GFT_LOCK(e);
    if (n_kept) *n_kept = 0;
    if (n_hits) *n_hits = 0;
    if (n_groups) *n_groups = 0;
    if (total_bytes) *total_bytes = 0;
    const uint32_t W = (n_cols + 31) / 32;
    if (n_docs && (!d_doc_off || !d_text_blob || (W && !d_bitmap))) return fail(e, GFT_E_INVALID, "null argument");
    if (cap_bytes && !d_out) return fail(e, GFT_E_INVALID, "gft_context_docs_device: cap_bytes but no output buffer");
    if (cap_docs && (!d_out_off || !d_doc_idx || !d_kind))
        return fail(e, GFT_E_INVALID, "gft_context_docs_device: cap_docs but no offset, index or kind array");
    if (cap_groups && !d_group_off) return fail(e, GFT_E_INVALID, "gft_context_docs_device: cap_groups but no group array");
    if (!e->peers.empty()) return fail(e, GFT_E_UNSUPPORTED, "gft_context_docs_device: single-device handles only");
    int rc = check_ready(e, kNeedDevice | kNeedSettled, "gft_context_docs_device");
    if (rc) return rc;
    if (mode != GFT_SELECT_ANY && mode != GFT_SELECT_ALL && mode != GFT_SELECT_NONE) return fail(e, GFT_E_INVALID, "gft_context_docs_device: unknown mode");
    if (cap_docs > (~0ull >> 4) || cap_groups > (~0ull >> 4) || n_docs > (~0ull >> 4))
        return fail(e, GFT_E_INVALID, "gft_context_docs_device: a size beyond the address space");
    DeviceGuard g(e->device);
    hipStream_t st = e->stream;
    if (!n_docs) return doc_gather_empty(e, kContext, d_out_off, d_group_off);
    auto& S = e->d_context;
    std::vector<uint32_t> h_want(std::max<uint32_t>(W, 1), 0);
    SyncOnExit drain(e);                                            // (h_want is handed to an asynchronous copy)
    select_want_words(want, n_cols, h_want.data());
    const uint64_t n_tiles = ctx_tiles(n_docs), n_blocks = ctx_blocks(n_tiles);
    if ((rc = room(e, S.want, (uint64_t)W * 4, kContext.room)) || (rc = room(e, S.sel, n_docs * 4, kContext.room)) ||
        (rc = room(e, S.len, n_docs * 4, kContext.room)) || (rc = room(e, S.keep, n_docs * 4, kContext.room)) ||
        (rc = room(e, S.word_sel, n_tiles * 8, kContext.room)) || (rc = room(e, S.word_fence, n_tiles * 8, kContext.room)) ||
        (rc = room(e, S.sum, n_tiles * 32, kContext.room)) || (rc = room(e, S.carry, n_tiles * 32, kContext.room)) ||
        (rc = room(e, S.part, n_blocks * 40, kContext.room)) || (rc = room(e, S.pos, (n_docs + 1) * 8, kContext.room)) ||
        (rc = room(e, S.rank, (n_docs + 1) * 8, kContext.room)) || (rc = room(e, S.grank, (n_docs + 1) * 8, kContext.room)) ||
        (rc = room(e, S.partial, scan_partials_needed(n_docs) * 8, kContext.room)) || (rc = room(e, S.ctl, kCtxCtlWords * 8, kContext.room)))
        return rc;
    ContextParams P{};
    P.doc_off = d_doc_off; P.n_docs = n_docs; P.n_tiles = n_tiles; P.n_blocks = n_blocks;
    P.sel = S.sel.as<uint32_t>(); P.fence = d_fence; P.before = before; P.after = after;
    P.word_sel = S.word_sel.as<uint64_t>(); P.word_fence = S.word_fence.as<uint64_t>(); P.sum = S.sum.as<uint64_t>();
    P.carry = S.carry.as<uint64_t>(); P.part = S.part.as<uint64_t>();
    P.keep = S.keep.as<uint32_t>(); P.len = S.len.as<uint32_t>();
    P.newgroup = S.sel.as<uint32_t>();                              // (the marks are in the tiles' words by then)
    P.pos = S.pos.as<uint64_t>(); P.rank = S.rank.as<uint64_t>(); P.grank = S.grank.as<uint64_t>(); P.ctl = S.ctl.as<uint64_t>();
    // the select's mark pass decides who is selected, and finds offsets that descend and documents of 4 GiB or more
    SelectParams M{};
    if ((rc = doc_gather_select_mark(e, kContext, M, d_text_blob, d_doc_off, n_docs, d_bitmap, n_cols, mode, d_also, h_want.data(), S.want, S.len, S.sel,
                                     S.ctl, kCtxCtlWords)))
        return rc;
    {
        ProfScope ps(e, "context_reach");
        HIP_TRY(launch_context_reach(P, e->n_cus, st), "context reach kernel launch");
    }
    {
        ProfScope ps(e, "context_carry");
        HIP_TRY(launch_context_carry(P, e->n_cus, st), "context carry kernel launch");
    }
    {
        ProfScope ps(e, "context_decide");
        HIP_TRY(launch_context_decide(P, e->n_cus, st), "context decide kernel launch");
    }
    {
        ProfScope ps(e, "context_scan");
        HIP_TRY(launch_exclusive_scan(P.len, n_docs, S.pos.as<uint64_t>(), S.partial.as<uint64_t>(), st), "context scan");
        HIP_TRY(launch_exclusive_scan(P.keep, n_docs, S.rank.as<uint64_t>(), S.partial.as<uint64_t>(), st), "context scan");
        HIP_TRY(launch_exclusive_scan(P.newgroup, n_docs, S.grank.as<uint64_t>(), S.partial.as<uint64_t>(), st), "context scan");
        HIP_TRY(launch_context_pack(P, st), "context scan");
    }
    uint64_t h_ctl[kCtxCtlWords] = {0};
    if ((rc = doc_gather_read(e, kContext, P.ctl, h_ctl, kCtxCtlWords))) return rc;
    if (context_buffers_overlap(d_text_blob, h_ctl[kSelCtlLo], h_ctl[kSelCtlHi], d_doc_off, n_docs, d_bitmap, n_cols, d_also, d_fence, d_out, cap_bytes,
                                d_out_off, d_doc_idx, d_kind, cap_docs, d_group_off, cap_groups))
        return doc_gather_overlap(e, kContext);
    P.total = h_ctl[kSelCtlTotal]; P.m = h_ctl[kSelCtlM]; P.groups = h_ctl[kCtxCtlGroups];
    if (n_kept) *n_kept = P.m;
    if (n_hits) *n_hits = h_ctl[kCtxCtlHits];
    if (n_groups) *n_groups = P.groups;
    if (total_bytes) *total_bytes = P.total;
    if ((rc = room(e, S.c_off, (P.m + 1) * 8, kContext.room)) || (rc = room(e, S.c_src, P.m * 8, kContext.room))) return rc;
    P.c_off = S.c_off.as<uint64_t>(); P.c_src = S.c_src.as<uint64_t>();
    P.out_off = d_out_off; P.doc_idx = d_doc_idx; P.kind = d_kind; P.cap_docs = cap_docs;
    P.group_off = d_group_off; P.cap_groups = cap_groups;
    {
        ProfScope ps(e, "context_place");
        HIP_TRY(launch_context_place(P, st), "context place kernel launch");
    }
    // the bytes: the select's copy pass over the compact arrays
    return doc_gather_copy(e, kContext, d_text_blob, P.c_off, P.c_src, P.m, P.total, d_out, cap_bytes);
} GFT_CATCH((e ? &e->err : nullptr))

int gft_debug_context_docs(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const uint32_t* bitmap, uint32_t n_cols,
                           const uint32_t* want, uint32_t mode, const uint8_t* also, uint64_t before, uint64_t after, const uint8_t* fence,
                           uint8_t* out, uint64_t cap_bytes, uint64_t* out_off, uint64_t* doc_idx, uint8_t* kind, uint64_t cap_docs,
                           uint64_t* group_off, uint64_t cap_groups, uint64_t* n_kept, uint64_t* n_hits, uint64_t* n_groups,
                           uint64_t* total_bytes) try {
    return context_docs_host(blob, doc_off, n_docs, bitmap, n_cols, want, mode, also, before, after, fence, out, cap_bytes, out_off, doc_idx, kind,
                             cap_docs, group_off, cap_groups, n_kept, n_hits, n_groups, total_bytes);
} GFT_CATCH(nullptr)

void gft_debug_context_shape(uint32_t* tile_docs, uint32_t* carry_block_tiles, uint32_t* spine_trip_blocks) {
    if (tile_docs) *tile_docs = kCtxTile;
    if (carry_block_tiles) *carry_block_tiles = kCtxCarry;
    if (spine_trip_blocks) *spine_trip_blocks = kCtxSpine;
}

}  // extern "C"
