// gft_tags_api.cpp -- tag entries of a record batch (gft_tags.hpp): the engine's side, which group_tags.cpp drives.
#include "gft_engine.hpp"

#include "gft_rules.hpp"
#include "gft_tags.hpp"

using namespace gft;
using namespace gft::api;

namespace {

constexpr RoomTexts kTagsRoom{"no device memory for the tag entries' work buffers", "tag entries alloc"};

struct TagOut {
    uint64_t* row_off; uint32_t* ent_field; uint32_t* ent_expr; uint32_t* ent_tag; uint64_t cap;
};

// count, scan, (owned: room for the total,) fill, flags.  out.row_off == nullptr: the engine's own arrays, returned in `out`.
int tag_entries(gft_engine* e, const uint32_t* d_hit_bitmap, const uint32_t* d_leaf_field, const uint64_t* d_rec_off, uint64_t n_records,
                uint64_t n_leaves, TagOut& out, bool owned, uint64_t* total) {
    if (!e->peers.empty()) return fail(e, GFT_E_UNSUPPORTED, "tag entries: single-device handles only");
    int rc = check_ready(e, kNeedDevice | kNeedSettled, "tag entries");
    if (rc) return rc;
    auto& R = e->d_rules;
    auto& T = e->d_tags;
    if (!R.serial) return fail(e, GFT_E_INVALID, "tag entries: no rule set installed");
    if (total) *total = 0;
    DeviceGuard g(e->device);
    hipStream_t st = e->stream;
    if (owned) {
        if ((rc = room(e, T.row_off, (n_records + 1) * 8, kTagsRoom)) || (rc = room(e, T.ent_field, 16, kTagsRoom)) || (rc = room(e, T.ent_expr, 16, kTagsRoom))) return rc;
        out = TagOut{T.row_off.as<uint64_t>(), T.ent_field.as<uint32_t>(), T.ent_expr.as<uint32_t>(), nullptr, 0};
    }
    if (!out.row_off) return fail(e, GFT_E_INVALID, "tag entries: null argument");
    if (out.cap && (!out.ent_field || !out.ent_expr)) return fail(e, GFT_E_INVALID, "tag entries: a cap but no array");
    if (!n_records) {
        if (n_leaves) return fail(e, GFT_E_INVALID, "record batch: leaves but no records");
        HIP_TRY(hipMemsetAsync(out.row_off, 0, 8, st), "tag entries");
        HIP_TRY(hipStreamSynchronize(st), "tag entries");
        return GFT_OK;
    }
    if (!d_rec_off || (n_leaves && (!d_leaf_field || (R.n_exprs && !d_hit_bitmap)))) return fail(e, GFT_E_INVALID, "record batch: null argument");
    if ((rc = room(e, T.cnt, n_leaves * 4, kTagsRoom)) || (rc = room(e, T.leaf_ent_off, (n_leaves + 1) * 8, kTagsRoom)) ||
        (rc = room(e, T.partial, scan_partials_needed(n_leaves) * 8, kTagsRoom)) || (rc = room(e, T.flags, 16, kTagsRoom)))
        return rc;
    TagParams P{};
    P.rows = bit_rows(d_hit_bitmap, n_leaves, R.n_exprs);
    P.leaf_field = d_leaf_field; P.valid = R.valid.as<uint32_t>(); P.n_fields = R.n_fields;
    P.flags = T.flags.as<uint32_t>(); P.cnt = T.cnt.as<uint32_t>();
    HIP_TRY(hipMemsetAsync(P.flags, 0, 8, st), "tag entries");
    {
        ProfScope ps(e, "tags_count");
        HIP_TRY(launch_tags_count(P, e->n_cus, st), "tag count kernel launch");
    }
    {
        ProfScope ps(e, "tags_scan");
        HIP_TRY(launch_exclusive_scan(P.cnt, n_leaves, T.leaf_ent_off.as<uint64_t>(), T.partial.as<uint64_t>(), st), "tag scan");
    }
    uint64_t h_total = 0;
    if (owned) {
        // (the one read that sizes the arrays; the caller's form reads the total with the flags, below)
        HIP_TRY(hipMemcpyAsync(&h_total, T.leaf_ent_off.as<uint64_t>() + n_leaves, 8, hipMemcpyDeviceToHost, st), "tag entries");
        HIP_TRY(hipStreamSynchronize(st), "tag entries");
        if ((rc = room(e, T.ent_field, h_total * 4, kTagsRoom)) || (rc = room(e, T.ent_expr, h_total * 4, kTagsRoom))) return rc;
        out.ent_field = T.ent_field.as<uint32_t>(); out.ent_expr = T.ent_expr.as<uint32_t>(); out.cap = h_total;
    }
    P.leaf_ent_off = T.leaf_ent_off.as<uint64_t>();
    P.rec_off = d_rec_off; P.n_records = n_records; P.row_off = out.row_off;
    P.ent_field = out.ent_field; P.ent_expr = out.ent_expr; P.ent_tag = out.ent_tag; P.expr_tag = R.expr_tag.as<uint32_t>();
    P.cap = out.cap;
    {
        ProfScope ps(e, "tags_fill");
        HIP_TRY(launch_tags_fill(P, e->n_cus, st), "tag fill kernel launch");
    }
    uint32_t h_flags[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(h_flags, P.flags, 8, hipMemcpyDeviceToHost, st), "tag entries");
    HIP_TRY(hipMemcpyAsync(&h_total, T.leaf_ent_off.as<uint64_t>() + n_leaves, 8, hipMemcpyDeviceToHost, st), "tag entries");
    HIP_TRY(hipStreamSynchronize(st), "tag entries");
    if ((rc = record_flags_rc(e, h_flags))) return rc;
    if (total) *total = h_total;           // (= row_off[n_records]: the offsets end at n_leaves)
    return GFT_OK;
}

}  // namespace

namespace gft {

int rules_tag_entries_device(gft_engine* e, const uint32_t* d_hit_bitmap, const uint32_t* d_leaf_field, const uint64_t* d_rec_off,
                             uint64_t n_records, uint64_t n_leaves, uint64_t* d_row_off, uint32_t* d_ent_field, uint32_t* d_ent_expr,
                             uint32_t* d_ent_tag, uint64_t cap, uint64_t* total) try {
    if (!e) return GFT_E_INVALID;
    GFT_LOCK(e);
    TagOut out{d_row_off, d_ent_field, d_ent_expr, cap ? d_ent_tag : nullptr, cap};
    return tag_entries(e, d_hit_bitmap, d_leaf_field, d_rec_off, n_records, n_leaves, out, false, total);
} GFT_CATCH((e ? &e->err : nullptr))

int rules_tag_entries_owned(gft_engine* e, const uint32_t* d_hit_bitmap, const uint32_t* d_leaf_field, const uint64_t* d_rec_off,
                            uint64_t n_records, uint64_t n_leaves, const uint64_t** d_row_off, const uint32_t** d_ent_field,
                            const uint32_t** d_ent_expr, uint64_t* total) try {
    if (!e || !d_row_off || !d_ent_field || !d_ent_expr || !total) return GFT_E_INVALID;
    GFT_LOCK(e);
    TagOut out{};
    int rc = tag_entries(e, d_hit_bitmap, d_leaf_field, d_rec_off, n_records, n_leaves, out, true, total);
    if (rc) return rc;
    *d_row_off = out.row_off; *d_ent_field = out.ent_field; *d_ent_expr = out.ent_expr;
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

}  // namespace gft
