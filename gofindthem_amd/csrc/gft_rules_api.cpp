// gft_rules_api.cpp -- rule evaluation for records (gft_rules.hpp): the engine's side, which group_records.cpp drives.
#include "gft_engine.hpp"

#include <atomic>

#include "gft_rules.hpp"
#include "rule_set.hpp"

using namespace gft;
using namespace gft::api;

namespace {
int rules_entry_checks(gft_engine* e) {
    if (!e->peers.empty()) return fail(e, GFT_E_UNSUPPORTED, "record batches: single-device handles only");
    return check_ready(e, kNeedDevice | kNeedSettled, "record batches");
}
constexpr RoomTexts kRulesRoom{"no device memory for the record batch's work buffers", "record batch alloc"};
}  // namespace

namespace gft {

int record_flags_rc(gft_engine* e, const uint32_t h_flags[2]) {
    if (h_flags[1]) return fail(e, GFT_E_INVALID, "record batch: rec_off descends or does not end at n_leaves");
    if (h_flags[0]) return fail(e, GFT_E_INVALID, "record batch: a leaf names a field outside the schema");
    return GFT_OK;
}

void rules_lock(gft_engine* e) { e->mu.lock(); }
void rules_unlock(gft_engine* e) { e->mu.unlock(); }

int rules_install(gft_engine* e, const RuleSet& rs, uint64_t* serial) try {
    if (!e || !serial) return GFT_E_INVALID;
    GFT_LOCK(e);
    int rc = rules_entry_checks(e);
    if (rc) return rc;
    if (rules_lds_bytes(rs.n_units(), rs.max_depth) + 64 > e->lds_max)
        return fail(e, GFT_E_UNSUPPORTED, "record rules: the UNIT words and operand stacks of this set do not fit the device's LDS");
    DeviceGuard g(e->device);
    auto& R = e->d_rules;
    R.serial = 0;                          // (a failed upload leaves no set)
    if ((rc = upload(e, R.expr_tag, rs.expr_tag, "rule set upload"))) return rc;
    if ((rc = upload(e, R.masks, rs.masks, "rule set upload"))) return rc;
    if ((rc = upload(e, R.units, rs.units, "rule set upload"))) return rc;
    if ((rc = upload(e, R.prog, rs.prog, "rule set upload"))) return rc;
    if ((rc = upload(e, R.prog_off, rs.prog_off, "rule set upload"))) return rc;
    if ((rc = upload(e, R.valid, rs.valid, "rule set upload"))) return rc;
    HIP_TRY(R.flags.ensure(16), "rule set upload");
    HIP_TRY(hipStreamSynchronize(e->stream), "rule set upload");
    R.n_fields = rs.n_fields; R.n_tags = rs.n_tags; R.n_exprs = rs.n_exprs; R.n_rules = rs.n_rules;
    R.n_units = rs.n_units(); R.max_depth = rs.max_depth; R.field_words = rs.field_words;
    static std::atomic<uint64_t> next_serial{1};
    *serial = R.serial = next_serial.fetch_add(1);
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

uint64_t rules_serial(gft_engine* e) {
    if (!e) return 0;
    GFT_LOCK(e);
    return e->d_rules.serial;
}

int rules_leaf_bitmap(gft_engine* e, uint64_t n_leaves, uint32_t words, uint32_t** d_bitmap) try {
    if (!e || !d_bitmap) return GFT_E_INVALID;
    GFT_LOCK(e);
    int rc = rules_entry_checks(e);
    if (rc) return rc;
    DeviceGuard g(e->device);
    if ((rc = room(e, e->d_rules.leaf_bitmap, n_leaves * words * 4, kRulesRoom))) return rc;
    *d_bitmap = e->d_rules.leaf_bitmap.as<uint32_t>();
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

int rules_stage(gft_engine* e, int n, const void* const* src, const uint64_t* bytes, const uint64_t* slack, void** d_dst) try {
    if (!e || n < 0 || n > 6 || (n && (!src || !bytes || !slack || !d_dst))) return GFT_E_INVALID;
    GFT_LOCK(e);
    int rc = rules_entry_checks(e);
    if (rc) return rc;
    DeviceGuard g(e->device);
    SyncOnExit drain(e);
    for (int k = 0; k < n; k++) {
        DevBuf& b = e->d_rules.stage[k];
        if ((rc = room(e, b, bytes[k] + slack[k], kRulesRoom))) return rc;
        if (bytes[k]) HIP_TRY(hipMemcpyAsync(b.p, src[k], bytes[k], hipMemcpyHostToDevice, e->stream), "record batch upload");
        if (slack[k]) HIP_TRY(hipMemsetAsync((uint8_t*)b.p + bytes[k], 0, slack[k], e->stream), "record batch upload");
        d_dst[k] = b.p;
    }
    HIP_TRY(hipStreamSynchronize(e->stream), "record batch upload");
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

int rules_fetch(gft_engine* e, void* dst, const void* d_src, uint64_t bytes) try {
    if (!e || (bytes && (!dst || !d_src))) return GFT_E_INVALID;
    GFT_LOCK(e);
    DeviceGuard g(e->device);
    SyncOnExit drain(e);
    if (bytes) HIP_TRY(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, e->stream), "rule bitmap download");
    HIP_TRY(hipStreamSynchronize(e->stream), "rule bitmap download");
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

int rules_eval_device(gft_engine* e, const uint32_t* d_hit_bitmap, const uint32_t* d_leaf_field, const uint64_t* d_rec_off,
                          uint64_t n_records, uint64_t n_leaves, uint32_t* d_rule_bitmap) try {
    if (!e) return GFT_E_INVALID;
    GFT_LOCK(e);
    int rc = rules_entry_checks(e);
    if (rc) return rc;
    auto& R = e->d_rules;
    if (!R.serial) return fail(e, GFT_E_INVALID, "record rules: no rule set installed");
    // (what validate_records refuses on the host is refused here: the kernels check fields and offsets also when no rule reads them)
    if (!n_records) return n_leaves ? fail(e, GFT_E_INVALID, "record batch: leaves but no records") : (int)GFT_OK;
    if (!d_rec_off || (R.n_rules && !d_rule_bitmap) || (n_leaves && (!d_leaf_field || (R.n_exprs && !d_hit_bitmap))))
        return fail(e, GFT_E_INVALID, "record batch: null argument");
    DeviceGuard g(e->device);
    hipStream_t st = e->stream;
    const uint32_t TW = (R.n_tags + 31) / 32;
    if ((rc = room(e, R.tag_rows, n_leaves * TW * 4, kRulesRoom))) return rc;
    uint32_t* d_flags = R.flags.as<uint32_t>();
    HIP_TRY(hipMemsetAsync(d_flags, 0, 8, st), "record rules");
    {
        ProfScope ps(e, "group_tags");
        HIP_TRY(launch_leaf_tags(d_hit_bitmap, R.n_exprs, R.expr_tag.as<uint32_t>(), d_leaf_field, R.n_fields, n_leaves, R.n_tags,
                                 R.tag_rows.as<uint32_t>(), d_flags, st), "leaf tag kernel launch");
    }
    RulesParams P{};
    P.tag_rows = R.tag_rows.as<uint32_t>();
    P.leaf_field = d_leaf_field;
    P.rec_off = d_rec_off;
    P.n_records = n_records; P.n_leaves = n_leaves;
    P.masks = R.masks.as<uint32_t>(); P.units = R.units.as<uint32_t>();
    P.prog = R.prog.as<uint32_t>(); P.prog_off = R.prog_off.as<uint32_t>();
    P.TW = TW; P.FW = R.field_words; P.RW = (R.n_rules + 31) / 32;
    P.n_fields = R.n_fields; P.n_units = R.n_units; P.n_rules = R.n_rules; P.max_depth = R.max_depth;
    P.flags = d_flags; P.out = d_rule_bitmap;
    {
        ProfScope ps(e, "group_rules");
        HIP_TRY(launch_record_rules(P, e->lds_max, st), "record rule kernel launch");
    }
    uint32_t h_flags[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(h_flags, d_flags, 8, hipMemcpyDeviceToHost, st), "record rules");
    HIP_TRY(hipStreamSynchronize(st), "record rules");
    return record_flags_rc(e, h_flags);
} GFT_CATCH((e ? &e->err : nullptr))

}  // namespace gft
