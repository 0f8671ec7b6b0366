// gft_result_api.cpp -- the result document of a batch's rule rows (gft_result.hpp): the engine's side, which group_json.cpp
// and gft_group_rules_json_device drive.
#include "gft_engine.hpp"

#include <atomic>

#include "gft_result.hpp"
#include "rules_json.hpp"

using namespace gft;
using namespace gft::api;

namespace {

constexpr RoomTexts kResultRoom{"no device memory for the result document's work buffers", "result document alloc"};

int result_entry_checks(gft_engine* e) {
    if (!e->peers.empty()) return fail(e, GFT_E_UNSUPPORTED, "result document: single-device handles only");
    return check_ready(e, kNeedDevice | kNeedSettled, "result document");
}

// count, scan, the total and the flags, (owned: room for the total,) fill.  d_out_off == nullptr: the engine's own arrays,
// returned in d_out / d_out_off.
int result_text(gft_engine* e, const uint32_t* d_rule_bitmap, uint64_t n_docs, const uint64_t* d_hole_len, uint8_t*& d_out, uint64_t cap,
                uint64_t*& d_out_off, bool owned, uint64_t* total) {
    int rc = result_entry_checks(e);
    if (rc) return rc;
    auto& T = e->d_result;
    if (!T.serial) return fail(e, GFT_E_INVALID, "result document: no fragment table installed");
    if (total) *total = 0;
    DeviceGuard g(e->device);
    hipStream_t st = e->stream;
    if (owned) {
        if ((rc = room(e, T.out_off, (n_docs + 1) * 8, kResultRoom))) return rc;
        d_out_off = T.out_off.as<uint64_t>();
    }
    if (!d_out_off) return fail(e, GFT_E_INVALID, "result document: null argument");
    if (!owned && cap && !d_out) return fail(e, GFT_E_INVALID, "result document: a cap but no text buffer");
    if (n_docs && T.n_exprs && !d_rule_bitmap) return fail(e, GFT_E_INVALID, "result document: null argument");
    if ((rc = room(e, T.cnt, n_docs * 4, kResultRoom)) || (rc = room(e, T.scan, (n_docs + 1) * 8, kResultRoom)) ||
        (rc = room(e, T.partial, scan_partials_needed(n_docs) * 8, kResultRoom)) || (rc = room(e, T.flags, 16, kResultRoom)))
        return rc;
    ResultParams P{};
    P.rows = d_rule_bitmap; P.n_docs = n_docs; P.R = T.n_exprs; P.RW = (T.n_exprs + 31) / 32;
    P.hole_len = d_hole_len;
    P.rule_first = T.rule_first.as<uint32_t>(); P.name_off = T.name_off.as<uint32_t>(); P.name_len = T.name_len.as<uint32_t>();
    P.expr_off = T.expr_off.as<uint32_t>(); P.expr_len = T.expr_len.as<uint32_t>(); P.blob = T.blob.as<uint8_t>();
    P.flags = T.flags.as<uint32_t>(); P.cnt = T.cnt.as<uint32_t>();
    uint64_t h_total = 1;                  // (n_docs == 0: "[]", with the closing bracket added below)
    if (n_docs) {
        HIP_TRY(hipMemsetAsync(P.flags, 0, 8, st), "result document");
        {
            ProfScope ps(e, "result_count");
            HIP_TRY(launch_result_count(P, e->n_cus, st), "result count kernel launch");
        }
        {
            ProfScope ps(e, "result_scan");
            HIP_TRY(launch_exclusive_scan(P.cnt, n_docs, T.scan.as<uint64_t>(), T.partial.as<uint64_t>(), st), "result scan");
        }
        // the one read between the passes: the total sizes the owned text, and a refused hole stops the call before the fill
        uint32_t h_flags[2] = {0, 0};
        HIP_TRY(hipMemcpyAsync(h_flags, P.flags, 8, hipMemcpyDeviceToHost, st), "result document");
        HIP_TRY(hipMemcpyAsync(&h_total, T.scan.as<uint64_t>() + n_docs, 8, hipMemcpyDeviceToHost, st), "result document");
        HIP_TRY(hipStreamSynchronize(st), "result document");
        if (h_flags[0]) return fail(e, GFT_E_INVALID, "result document: a hole of 4 GiB or more");
    }
    h_total += 1;                          // the opening bracket
    if (owned) {
        if ((rc = room(e, T.text, h_total, kResultRoom))) return rc;
        d_out = T.text.as<uint8_t>();
        cap = h_total;
    }
    P.scan = T.scan.as<uint64_t>(); P.out_off = d_out_off; P.out = d_out; P.cap = d_out ? cap : 0;
    {
        ProfScope ps(e, "result_fill");
        HIP_TRY(launch_result_fill(P, e->n_cus, st), "result fill kernel launch");
    }
    HIP_TRY(hipStreamSynchronize(st), "result document");
    if (total) *total = h_total;
    return GFT_OK;
}

}  // namespace

namespace gft {

int rules_json_install(gft_engine* e, const RuleFragments& fr, uint64_t* serial) try {
    if (!e || !serial) return GFT_E_INVALID;
    GFT_LOCK(e);
    int rc = result_entry_checks(e);
    if (rc) return rc;
    DeviceGuard g(e->device);
    auto& T = e->d_result;
    T.serial = 0;                          // (a failed upload leaves no table)
    if ((rc = upload(e, T.rule_first, fr.rule_first, "fragment table upload")) || (rc = upload(e, T.name_off, fr.name_off, "fragment table upload")) ||
        (rc = upload(e, T.name_len, fr.name_len, "fragment table upload")) || (rc = upload(e, T.expr_off, fr.expr_off, "fragment table upload")) ||
        (rc = upload(e, T.expr_len, fr.expr_len, "fragment table upload")) || (rc = upload(e, T.blob, fr.blob, "fragment table upload")))
        return rc;
    HIP_TRY(hipStreamSynchronize(e->stream), "fragment table upload");
    T.n_exprs = fr.n_exprs();
    static std::atomic<uint64_t> next_serial{1};
    *serial = T.serial = next_serial.fetch_add(1);
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

uint64_t rules_json_serial(gft_engine* e) {
    if (!e) return 0;
    GFT_LOCK(e);
    return e->d_result.serial;
}

int rules_json_device(gft_engine* e, const uint32_t* d_rule_bitmap, uint64_t n_docs, const uint64_t* d_hole_len, uint8_t* d_out, uint64_t cap,
                      uint64_t* d_out_off, uint64_t* total) try {
    if (!e) return GFT_E_INVALID;
    GFT_LOCK(e);
    return result_text(e, d_rule_bitmap, n_docs, d_hole_len, d_out, cap, d_out_off, false, total);
} GFT_CATCH((e ? &e->err : nullptr))

int rules_json_owned(gft_engine* e, const uint32_t* d_rule_bitmap, uint64_t n_docs, const uint64_t* h_hole_len, const uint8_t** d_text,
                     const uint64_t** d_out_off, uint64_t* total) try {
    if (!e || !d_text || !d_out_off || !total) return GFT_E_INVALID;
    GFT_LOCK(e);
    int rc = result_entry_checks(e);
    if (rc) return rc;
    const uint64_t* d_hole_len = nullptr;
    if (h_hole_len && n_docs) {
        DeviceGuard g(e->device);
        SyncOnExit drain(e);
        if ((rc = room(e, e->d_result.hole_len, n_docs * 8, kResultRoom))) return rc;
        HIP_TRY(hipMemcpyAsync(e->d_result.hole_len.p, h_hole_len, n_docs * 8, hipMemcpyHostToDevice, e->stream), "hole lengths upload");
        HIP_TRY(hipStreamSynchronize(e->stream), "hole lengths upload");
        d_hole_len = e->d_result.hole_len.as<uint64_t>();
    }
    uint8_t* out = nullptr;
    uint64_t* off = nullptr;
    if ((rc = result_text(e, d_rule_bitmap, n_docs, d_hole_len, out, 0, off, true, total))) return rc;
    *d_text = out; *d_out_off = off;
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

}  // namespace gft
