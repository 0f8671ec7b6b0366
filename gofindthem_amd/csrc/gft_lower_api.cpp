// gft_lower_api.cpp -- strings.ToLower of a batch on the device (gft_tolower.hip): gft_to_lower_device, gft_lower_owned.
#include "gft_engine.hpp"
#include "gft_tolower.hpp"

using namespace gft;
using namespace gft::api;

namespace gft::api {

// strings.ToLower of a batch, first half: the unit table, the count pass, the prefix sum and d_out_off (complete when this
// returns GFT_OK; the stream has drained).  *n_units / *total: what lower_write needs and what the caller sizes its buffer by.
// d_out / cap take part in the overlap check only.  (gft_engine.hpp: gft_lowermap_api.cpp builds its table on these passes.)
int lower_count(gft_engine* e, const uint8_t* d_text, const uint64_t* d_doc_off, uint64_t n_docs, const uint8_t* d_out, uint64_t cap,
                uint64_t* d_out_off, uint64_t* n_units, uint64_t* total, const char* who, const char* stage, uint64_t* text_range) {
    hipStream_t st = e->stream;
    const std::string me(who);
    *n_units = 0; *total = 0;
    if (text_range) text_range[0] = text_range[1] = 0;
    if (!n_docs) {
        HIP_TRY(hipMemsetAsync(d_out_off, 0, 8, st), "lower offsets");
        HIP_TRY(hipStreamSynchronize(st), "lower offsets");
        return GFT_OK;
    }
    if (!e->d_lw.table_up) {
        const LowerTableHost& t = lower_table_host();
        int rc = upload(e, e->d_lw.page, t.page, "lower table upload");
        if (!rc) rc = upload(e, e->d_lw.delta, t.delta, "lower table upload");
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(st), "lower table upload");
        e->d_lw.table_up = true;
    }
    const LowerTable T{e->d_lw.page.as<uint16_t>(), e->d_lw.delta.as<int32_t>(), (uint32_t)lower_table_host().page.size()};
    // d_lw.ctl: [0] units, [1] first and [2] last text offset (k_pack_ctl), [3] flags: 1 a document of 4 GiB or more or
    // descending offsets (k_unit_count), 2 a lowered document of 4 GiB or more (k_lower_offsets)
    HIP_TRY(e->d_lw.ctl.ensure(32), "lower alloc");
    HIP_TRY(e->d_lw.doc_units.ensure(n_docs * 4), "lower alloc");
    HIP_TRY(e->d_lw.unit_base.ensure((n_docs + 1) * 8), "lower alloc");
    HIP_TRY(e->d_lw.partial.ensure(scan_partials_needed(n_docs) * 8), "lower alloc");
    uint64_t* ctl = e->d_lw.ctl.as<uint64_t>();
    uint32_t* flags = reinterpret_cast<uint32_t*>(ctl + 3);
    uint64_t h_ctl[4] = {0, 0, 0, 0};
    {
        ProfScope ps(e, "aux");
        HIP_TRY(hipMemsetAsync(ctl, 0, 32, st), "lower units");
        HIP_TRY(launch_unit_count(d_doc_off, n_docs, kLowerUnitMax, e->d_lw.doc_units.as<uint32_t>(), flags, st), "lower units");
        HIP_TRY(launch_exclusive_scan(e->d_lw.doc_units.as<uint32_t>(), n_docs, e->d_lw.unit_base.as<uint64_t>(), e->d_lw.partial.as<uint64_t>(), st),
                "lower units");
        HIP_TRY(launch_pack_ctl(e->d_lw.unit_base.as<uint64_t>(), d_doc_off, n_docs, ctl, st), "lower units");
    }
    HIP_TRY(hipMemcpyAsync(h_ctl, ctl, 32, hipMemcpyDeviceToHost, st), "lower units");
    HIP_TRY(hipStreamSynchronize(st), "lower units");
    if (h_ctl[3] & 1) return fail(e, GFT_E_INVALID, me + ": document offsets descend, or a document of 4 GiB or more");
    if (lower_buffers_overlap(d_text, h_ctl[1], h_ctl[2], d_doc_off, n_docs, d_out, cap, d_out_off))
        return fail(e, GFT_E_INVALID, me + ": the output overlaps the input");
    if (text_range) { text_range[0] = h_ctl[1]; text_range[1] = h_ctl[2]; }
    const uint64_t nu = h_ctl[0];
    HIP_TRY(e->d_lw.units.ensure(nu * sizeof(Unit)), "lower alloc");
    HIP_TRY(e->d_lw.unit_cnt.ensure(nu * 4), "lower alloc");
    HIP_TRY(e->d_lw.unit_out.ensure((nu + 1) * 8), "lower alloc");
    HIP_TRY(e->d_lw.partial.ensure(scan_partials_needed(nu) * 8), "lower alloc");
    {
        ProfScope ps(e, "aux");
        HIP_TRY(launch_unit_fill(d_doc_off, n_docs, e->d_lw.unit_base.as<uint64_t>(), e->d_lw.units.as<Unit>(), kLowerUnitMax, st, nu), "lower units");
    }
    {
        ProfScope ps(e, stage ? stage : "lower_count");
        HIP_TRY(launch_lower_count(d_text, d_doc_off, e->d_lw.units.as<Unit>(), nu, T, e->d_lw.unit_cnt.as<uint32_t>(), e->n_cus, st), "lower count");
    }
    {
        ProfScope ps(e, stage ? stage : "lower_scan");
        HIP_TRY(launch_exclusive_scan(e->d_lw.unit_cnt.as<uint32_t>(), nu, e->d_lw.unit_out.as<uint64_t>(), e->d_lw.partial.as<uint64_t>(), st), "lower scan");
        HIP_TRY(launch_lower_offsets(e->d_lw.unit_base.as<uint64_t>(), e->d_lw.unit_out.as<uint64_t>(), n_docs, d_out_off, flags, st), "lower scan");
    }
    HIP_TRY(hipMemcpyAsync(h_ctl, e->d_lw.unit_out.as<uint64_t>() + nu, 8, hipMemcpyDeviceToHost, st), "lower total");
    HIP_TRY(hipMemcpyAsync(h_ctl + 3, ctl + 3, 8, hipMemcpyDeviceToHost, st), "lower total");
    HIP_TRY(hipStreamSynchronize(st), "lower count");
    if (h_ctl[3] & 2) return fail(e, GFT_E_INVALID, me + ": the lower-case form of a document has 4 GiB or more");
    *n_units = nu; *total = h_ctl[0];
    return GFT_OK;
}

}  // namespace gft::api

namespace {

// ... second half: the write pass over the unit table and prefix sums lower_count left in the engine.  Nothing waits here.
int lower_write(gft_engine* e, const uint8_t* d_text, const uint64_t* d_doc_off, uint64_t n_units, uint8_t* d_out, uint64_t cap) {
    if (!n_units || !cap) return GFT_OK;
    const LowerTable T{e->d_lw.page.as<uint16_t>(), e->d_lw.delta.as<int32_t>(), (uint32_t)lower_table_host().page.size()};
    ProfScope ps(e, "lower_write");
    HIP_TRY(launch_lower_write(d_text, d_doc_off, e->d_lw.units.as<Unit>(), n_units, T, e->d_lw.unit_out.as<uint64_t>(), d_out, cap, e->n_cus,
                               e->stream), "lower write");
    return GFT_OK;
}

int lower_entry_checks(gft_engine* e, const char* who) {
    if (!e->peers.empty()) return fail(e, GFT_E_UNSUPPORTED, std::string(who) + ": single-device handles only");
    return check_ready(e, kNeedDevice | kNeedSettled, who);
}

}  // namespace

extern "C" {

int gft_to_lower_device(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint8_t* d_out, uint64_t cap,
                        uint64_t* d_out_off, uint64_t* total) try {
    if (!e || !d_out_off || (n_docs && !d_doc_off)) return e ? fail(e, GFT_E_INVALID, "null argument") : GFT_E_INVALID;
    GFT_LOCK(e);
    if (cap && !d_out) return fail(e, GFT_E_INVALID, "gft_to_lower_device: cap bytes but no output buffer");
    int rc = lower_entry_checks(e, "gft_to_lower_device");
    if (rc) return rc;
    DeviceGuard g(e->device);
    uint64_t n_units = 0, n_total = 0;
    if ((rc = lower_count(e, d_text_blob, d_doc_off, n_docs, d_out, cap, d_out_off, &n_units, &n_total, "gft_to_lower_device"))) return rc;
    if (total) *total = n_total;
    if ((rc = lower_write(e, d_text_blob, d_doc_off, n_units, d_out, cap))) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream), "lower write");
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

int gft_lower_owned(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs, const uint8_t** d_lowered,
                    const uint64_t** d_lowered_off) try {
    if (!e || !d_lowered || !d_lowered_off || (n_docs && !d_doc_off)) return e ? fail(e, GFT_E_INVALID, "null argument") : GFT_E_INVALID;
    GFT_LOCK(e);
    int rc = lower_entry_checks(e, "lowering a batch");
    if (rc) return rc;
    DeviceGuard g(e->device);
    auto room = [&](DevBuf& b, uint64_t bytes) {
        const hipError_t h = b.ensure(bytes);
        if (h == hipErrorOutOfMemory) { (void)hipGetLastError(); return fail(e, GFT_E_NOMEM, "no device memory for the lowered batch"); }
        return h == hipSuccess ? (int)GFT_OK : fail_hip(e, h, "lower alloc");
    };
    if ((rc = room(e->d_lw.off, (n_docs + 1) * 8))) return rc;
    uint64_t n_units = 0, total = 0;
    if ((rc = lower_count(e, d_text_blob, d_doc_off, n_docs, nullptr, 0, e->d_lw.off.as<uint64_t>(), &n_units, &total, "gft_to_lower_device"))) return rc;
    if ((rc = room(e->d_lw.text, total + 64))) return rc;
    if ((rc = lower_write(e, d_text_blob, d_doc_off, n_units, e->d_lw.text.as<uint8_t>(), total))) return rc;
    *d_lowered = e->d_lw.text.as<uint8_t>();
    *d_lowered_off = e->d_lw.off.as<uint64_t>();
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

}  // extern "C"
