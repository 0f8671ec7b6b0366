// gft_process.cpp -- the batch entry points of include/gft.h: gft_scan*, gft_process* (two batches in flight included),
// gft_process_again, the sparse results.  They stage, call the pipelines of gft_pipeline.cpp and publish the verdict.
#include "gft_engine.hpp"

#include <chrono>
#include <cstdio>
#include <cstdlib>

#include "compact_host.hpp"

using namespace gft;
using namespace gft::api;

// What gft_scan / gft_scan_device do behind the scan itself: GFT_SCAN_UNIQUE, GFT_POS_RUNES, the non-ASCII verdict
static int scan_post(gft_engine* e, const uint8_t* d_text, const uint64_t* d_doc_off, uint64_t n_docs, uint32_t flags, uint64_t& nm,
                     BatchVerdict& v) {
    int rc;
    if ((flags & GFT_SCAN_UNIQUE) && (rc = unique_pipeline(e, n_docs, &nm))) return rc;
    if ((flags & GFT_POS_RUNES) && !(flags & GFT_SCAN_UNIQUE)) {
        if (e->build_flags & GFT_POS_END) return fail(e, GFT_E_UNSUPPORTED, "GFT_POS_RUNES needs a GFT_POS_START engine (AnknownEngine reports where a match begins)");
        if ((rc = rune_pipeline(e, d_text, d_doc_off, n_docs, nm))) return rc;
    }
    return refine_nonascii(e, d_text, d_doc_off, n_docs, flags, v);
}

extern "C" {

int gft_scan_device(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs,
                    uint32_t flags, gft_matches* out_dev) try {
    if (!e || !out_dev || (n_docs && (!d_text_blob || !d_doc_off))) return e ? fail(e, GFT_E_INVALID, "null argument") : GFT_E_INVALID;
    GFT_LOCK(e);
    if (int rc = check_ready(e, kNeedDevice | kNeedBuilt)) return rc;
    DeviceGuard g(e->device);
    BatchVerdict v;
    Publish publish{e, v};
    int rc = scan_pipeline(e, d_text_blob, d_doc_off, n_docs, flags, true, v);
    if (rc) return rc;
    uint64_t nm = v.total;
    if ((rc = scan_post(e, d_text_blob, d_doc_off, n_docs, flags, nm, v))) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream), "scan pipeline");
    out_dev->n_docs = n_docs; out_dev->n_matches = nm;
    out_dev->match_off = e->d_match_off.as<uint64_t>();
    out_dev->term_id = e->d_term.as<uint32_t>();
    out_dev->pos = e->d_pos.as<uint32_t>();
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

int gft_scan(gft_engine* e, const uint8_t* text_blob, const uint64_t* doc_off, uint64_t n_docs, uint32_t flags,
             gft_matches* out) try {
    if (!e || !out || (n_docs && (!doc_off))) return e ? fail(e, GFT_E_INVALID, "null argument") : GFT_E_INVALID;
    GFT_LOCK(e);
    if (!e->peers.empty() && !e->in_multi && n_docs) return multi_scan(e, text_blob, doc_off, n_docs, flags, out);   // (an empty batch -- doc_off may be NULL -- is the first device's)
    if (int rc = check_ready(e, kNeedDevice | kNeedBuilt)) return rc;
    DeviceGuard g(e->device);
    SyncOnExit drained(e);      // host buffers are read by asynchronous copies: drained on every way out
    int rc = stage_docs(e, text_blob, doc_off, n_docs);
    if (rc) return rc;
    BatchVerdict v;
    Publish publish{e, v};
    rc = scan_pipeline(e, e->d_text.as<uint8_t>(), e->d_doc_off.as<uint64_t>(), n_docs, flags, true, v, doc_off);
    if (rc) return rc;
    uint64_t nm = v.total;
    if ((rc = scan_post(e, e->d_text.as<uint8_t>(), e->d_doc_off.as<uint64_t>(), n_docs, flags, nm, v))) return rc;
    e->h_match_off.assign(n_docs + 1, 0);
    e->h_term.assign(nm, 0);
    e->h_pos.assign(nm, 0);
    HIP_TRY(hipMemcpyAsync(e->h_match_off.data(), e->d_match_off.p, (n_docs + 1) * 8, hipMemcpyDeviceToHost, e->stream), "download");
    if (nm) {
        HIP_TRY(hipMemcpyAsync(e->h_term.data(), e->d_term.p, nm * 4, hipMemcpyDeviceToHost, e->stream), "download");
        HIP_TRY(hipMemcpyAsync(e->h_pos.data(), e->d_pos.p, nm * 4, hipMemcpyDeviceToHost, e->stream), "download");
    }
    HIP_TRY(hipStreamSynchronize(e->stream), "scan pipeline");
    out->n_docs = n_docs; out->n_matches = nm;
    out->match_off = e->h_match_off.data(); out->term_id = e->h_term.data(); out->pos = e->h_pos.data();
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

namespace {
// the seven-word read-back of the control block into a pinned slot, enqueued behind a batch's last kernel (into pinned
// memory: a copy to pageable memory is staged by the runtime, ten microseconds on every batch)
int enqueue_ctl_readback(gft_engine* e, uint64_t** slot) {
    if (!*slot) HIP_TRY(hipHostMalloc((void**)slot, kCtlBytes, hipHostMallocDefault), "pinned alloc");
    HIP_TRY(hipMemcpyAsync(*slot, e->d_ctl.p, kCtlWords * sizeof(uint64_t), hipMemcpyDeviceToHost, e->stream), "readback");
    return GFT_OK;
}

// gft_process_device behind its lock and its in-flight guard: one batch from start to end, with its own synchronisations;
// `v` = its verdict.  It reuses the control block, so its callers inside _begin / _end / _complete have every older
// deferred batch's read-back on the host before they call.  They keep a status per batch: the function-try-block.
int process_device_sync(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint32_t flags,
                        const gft_extra_matches* d_extra, uint32_t* d_hit_bitmap, BatchVerdict& v) try {
    if (int rc = check_ready(e, kNeedDevice | kNeedBuilt | kNeedPrograms)) return rc;
    if (n_docs && e->n_exprs && !d_hit_bitmap) return fail(e, GFT_E_INVALID, "null bitmap");
    DeviceGuard g(e->device);
    // what the host solves (normally nothing): expressions beyond the device solver's limits, and INORD expressions in
    // documents where the caller's matches make a slot's list non-ascending -- for that the caller's (device) arrays are
    // read back, but only when some INORD group could be affected at all
    HostPlan plan;
    std::vector<uint64_t> xo;
    std::vector<uint32_t> xs, xp;
    gft_extra_matches hx{nullptr, nullptr, nullptr};
    const bool want_hx = d_extra && d_extra->off && n_docs && (!e->progs.host_only.empty() || !e->progs.inord_exprs.empty());
    if (want_hx) {
        xo.resize(n_docs + 1);
        HIP_TRY(hipMemcpy(xo.data(), d_extra->off, (n_docs + 1) * 8, hipMemcpyDeviceToHost), "extra read-back");
        // (the host walks these arrays now, not only the kernel: offsets must ascend, slots must exist -- what upload_extra
        // checks for host arrays)
        for (uint64_t d = 0; d < n_docs; d++)
            if (xo[d] > xo[d + 1]) return fail(e, GFT_E_INVALID, "extra offsets are not ascending");
        if (xo[n_docs] > (1ull << 40)) return fail(e, GFT_E_INVALID, "extra offsets are out of range");
        xs.resize(xo[n_docs] + 1); xp.resize(xo[n_docs] + 1);
        if (xo[n_docs]) {
            HIP_TRY(hipMemcpy(xs.data(), d_extra->slot, xo[n_docs] * 4, hipMemcpyDeviceToHost), "extra read-back");
            HIP_TRY(hipMemcpy(xp.data(), d_extra->pos, xo[n_docs] * 4, hipMemcpyDeviceToHost), "extra read-back");
            const uint64_t n_slots = e->tables.tab.terms.size() + e->n_extra;
            for (uint64_t i = xo[0]; i < xo[n_docs]; i++)
                if (xs[i] >= n_slots) return fail(e, GFT_E_INVALID, "extra slot out of range");
        }
        hx.off = xo.data(); hx.slot = xs.data(); hx.pos = xp.data();
    }
    plan_host(e, want_hx ? &hx : nullptr, n_docs, plan);
    // units -> scan -> solve without a host round trip in between; one read-back at the end, and a second pass only when
    // this batch outgrew the unit table or the match pool the previous ones left behind
    for (int pass = 0; pass < 2; pass++) {
        ScanLaunch launch;
        int rc = scan_pipeline(e, d_text_blob, d_doc_off, n_docs, flags, plan.all_docs, v, nullptr, pass == 0 ? &launch : nullptr);
        if (rc) return rc;
        rc = solve_pipeline(e, n_docs, d_extra, d_hit_bitmap);
        if (rc) return rc;
        if (!launch.deferred) break;
        if ((rc = enqueue_ctl_readback(e, &e->pin_rb))) return rc;
        HIP_TRY(hipStreamSynchronize(e->stream), "process pipeline");
        bool again = false;
        rc = deferred_interpret(e, e->pin_rb, launch, v, &again);
        if (rc) return rc;
        if (!again) break;
    }
    HIP_TRY(hipStreamSynchronize(e->stream), "process pipeline");
    int rc = refine_nonascii(e, d_text_blob, d_doc_off, n_docs, flags, v);
    if (rc) return rc;
    return host_eval(e, want_hx ? &hx : nullptr, n_docs, plan, nullptr, d_hit_bitmap);
} GFT_CATCH(&e->err)
}  // namespace

int gft_process_device(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs,
                       uint32_t flags, const gft_extra_matches* d_extra, uint32_t* d_hit_bitmap) try {
    if (!e || (n_docs && (!d_text_blob || !d_doc_off))) return e ? fail(e, GFT_E_INVALID, "null argument") : GFT_E_INVALID;
    GFT_LOCK(e);
    if (int rc = check_ready(e, kNeedSettled)) return rc;
    BatchVerdict v;
    const int rc = process_device_sync(e, d_text_blob, d_doc_off, n_docs, flags, d_extra, d_hit_bitmap, v);
    e->reported = v;
    return rc;
} GFT_CATCH((e ? &e->err : nullptr))

// ---- two batches in flight (at 125 000 documents -- one GPU's share of 1 M over 8 -- a step is 0.5 ms of
// kernels, and the read-back of the control block plus the launches of the next step are a tenth of it) -----------------------
namespace {
// a batch in flight is complete: its status is kept in its slot, beside its verdict, until its _end
void settle(gft_engine::Pending& p, int rc) { p.rc = rc; p.done = true; }
// Completes a deferred batch in place: the wait for its read-back, its verdict, and a second run when it outgrew the unit
// table or the match pool it was launched with.  `young`: the batch begun after it, still in flight behind it on the stream
// -- its read-back must have landed before a second run reuses the control block.
void complete_pending(gft_engine* e, gft_engine::Pending& p, gft_engine::Pending* young) {
    if (p.done) return;
    if (hipEventSynchronize(p.ev) != hipSuccess) { settle(p, fail(e, GFT_E_HIP, "event wait")); return; }
    bool again = false;
    int rc = deferred_interpret(e, p.rb, p.launch, p.verdict, &again);
    if (!rc && again) {
        if (young && !young->done && hipEventSynchronize(young->ev) != hipSuccess) { settle(p, fail(e, GFT_E_HIP, "event wait")); return; }
        rc = process_device_sync(e, p.d_text, p.d_doc_off, p.n_docs, p.flags, nullptr, p.d_bitmap, p.verdict);
    } else if (!rc) {
        rc = refine_nonascii(e, p.d_text, p.d_doc_off, p.n_docs, p.flags, p.verdict);
    }
    settle(p, rc);
}
}  // namespace

int gft_process_device_begin(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs,
                             uint32_t flags, const gft_extra_matches* d_extra, uint32_t* d_hit_bitmap) try {
    if (!e || (n_docs && (!d_text_blob || !d_doc_off))) return e ? fail(e, GFT_E_INVALID, "null argument") : GFT_E_INVALID;
    GFT_LOCK(e);
    if (!e->peers.empty()) return fail(e, GFT_E_UNSUPPORTED, "gft_process_device_begin: single-device handles only");
    if (e->pend_count == 2) return fail(e, GFT_E_INVALID, "gft_process_device_begin: two batches are in flight already (gft_process_device_end first)");
    const unsigned k = (e->pend_head + e->pend_count) % 2;
    gft_engine::Pending& pb = e->pend[k];
    pb.done = false; pb.rc = GFT_OK; pb.verdict = BatchVerdict();
    pb.d_text = d_text_blob; pb.d_doc_off = d_doc_off; pb.n_docs = n_docs; pb.flags = flags; pb.d_bitmap = d_hit_bitmap;
    const bool simple = n_docs && e->device >= 0 && e->built && e->have_programs && !(d_extra && d_extra->off) && e->progs.host_only.empty() &&
                        (!e->n_exprs || d_hit_bitmap);
    if (!simple) {
        // (whatever cannot be deferred -- caller-supplied matches, host-solved expressions, the first batches of an engine,
        // an empty batch -- completes here; _end then only hands its status and verdict back.  A batch before it is
        // completed first: the synchronous path reuses the control block it is still to read)
        if (e->pend_count) { DeviceGuard g2(e->device); complete_pending(e, e->pend[e->pend_head], nullptr); }
        settle(pb, process_device_sync(e, d_text_blob, d_doc_off, n_docs, flags, d_extra, d_hit_bitmap, pb.verdict));
        e->pend_count++;
        return GFT_OK;
    }
    DeviceGuard g(e->device);
    int rc = scan_pipeline(e, d_text_blob, d_doc_off, n_docs, flags, false, pb.verdict, nullptr, &pb.launch);
    if (rc) { settle(pb, rc); e->pend_count++; return GFT_OK; }
    rc = solve_pipeline(e, n_docs, nullptr, d_hit_bitmap);
    if (rc || !pb.launch.deferred) {
        // (sizes were not known yet: this batch ran with its own synchronisations, like gft_process_device's first pass)
        if (!rc) { rc = hipStreamSynchronize(e->stream) == hipSuccess ? GFT_OK : fail(e, GFT_E_HIP, "process pipeline"); }
        if (!rc) rc = refine_nonascii(e, d_text_blob, d_doc_off, n_docs, flags, pb.verdict);
        settle(pb, rc);
        e->pend_count++;
        return GFT_OK;
    }
    if (!pb.ev) HIP_TRY(hipEventCreateWithFlags(&pb.ev, hipEventDisableTiming), "event");
    if ((rc = enqueue_ctl_readback(e, &pb.rb))) return rc;
    HIP_TRY(hipEventRecord(pb.ev, e->stream), "event");
    e->pend_count++;
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

int gft_process_device_end(gft_engine* e) try {
    if (!e) return GFT_E_INVALID;
    GFT_LOCK(e);
    if (!e->pend_count) return fail(e, GFT_E_INVALID, "gft_process_device_end: no batch in flight");
    gft_engine::Pending& pb = e->pend[e->pend_head];
    if (!pb.done) {
        // a batch that outgrew the unit table or the match pool (both have been grown) runs once more here, with its own
        // synchronisations.  A younger batch in flight is behind it on the stream; it keeps its own bitmap and verdict.
        DeviceGuard g(e->device);
        complete_pending(e, pb, e->pend_count == 2 ? &e->pend[(e->pend_head + 1) % 2] : nullptr);
    }
    e->reported = pb.verdict;
    const int rc = pb.rc;
    e->pend_head = (e->pend_head + 1) % 2;
    e->pend_count--;
    return rc;
} GFT_CATCH((e ? &e->err : nullptr))

int gft_process_device_complete(gft_engine* e) try {
    if (!e) return GFT_E_INVALID;
    GFT_LOCK(e);
    if (pend_settled(e)) return GFT_OK;
    DeviceGuard g(e->device);
    // (every batch keeps its status and its verdict for its own _end; what gft_last_nonascii says stays)
    for (unsigned i = 0; i < e->pend_count; i++)
        complete_pending(e, e->pend[(e->pend_head + i) % 2], i + 1 < e->pend_count ? &e->pend[(e->pend_head + i + 1) % 2] : nullptr);
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

namespace {
// caller-supplied matches (host arrays) -> device copies; pdx stays null when there are none
int upload_extra(gft_engine* e, const gft_extra_matches* extra, uint64_t n_docs, gft_extra_matches& dx, const gft_extra_matches*& pdx) {
    pdx = nullptr;
    if (!(extra && extra->off && n_docs)) return GFT_OK;
    const uint64_t nx = extra->off[n_docs];
    HIP_TRY(e->d_xoff.ensure((n_docs + 1) * 8), "extra alloc");
    HIP_TRY(e->d_xslot.ensure(std::max<uint64_t>(nx, 1) * 4), "extra alloc");
    HIP_TRY(e->d_xpos.ensure(std::max<uint64_t>(nx, 1) * 4), "extra alloc");
    HIP_TRY(hipMemcpyAsync(e->d_xoff.p, extra->off, (n_docs + 1) * 8, hipMemcpyHostToDevice, e->stream), "extra upload");
    if (nx) {
        for (uint64_t i = 0; i < nx; i++)
            if (extra->slot[i] >= e->tables.tab.terms.size() + e->n_extra) return fail(e, GFT_E_INVALID, "extra slot out of range");
        HIP_TRY(hipMemcpyAsync(e->d_xslot.p, extra->slot, nx * 4, hipMemcpyHostToDevice, e->stream), "extra upload");
        HIP_TRY(hipMemcpyAsync(e->d_xpos.p, extra->pos, nx * 4, hipMemcpyHostToDevice, e->stream), "extra upload");
    }
    dx.off = e->d_xoff.as<uint64_t>(); dx.slot = e->d_xslot.as<uint32_t>(); dx.pos = e->d_xpos.as<uint32_t>();
    pdx = &dx;
    return GFT_OK;
}
}  // namespace

int gft_process_again(gft_engine* e, uint64_t n_docs, const gft_extra_matches* extra, uint32_t* hit_bitmap) try {
    if (!e) return GFT_E_INVALID;
    GFT_LOCK(e);
    if (!e->peers.empty() && !e->in_multi) return multi_process_again(e, n_docs, extra, hit_bitmap);
    if (int rc = check_ready(e, kNeedDevice)) return rc;
    if (!e->built || !e->have_programs) return fail(e, GFT_E_NOT_BUILT, "engine not ready");
    if (e->pool.valid_docs != n_docs || !n_docs) return fail(e, GFT_E_INVALID, "gft_process_again: no scan of these documents to reuse");
    DeviceGuard g(e->device);
    SyncOnExit drained(e);      // host buffers are read by asynchronous copies: drained on every way out
    gft_extra_matches dx;
    const gft_extra_matches* pdx = nullptr;
    int rc = upload_extra(e, extra, n_docs, dx, pdx);
    if (rc) return rc;
    const uint64_t words = (e->n_exprs + 31) / 32;
    HostPlan plan;
    plan_host(e, pdx ? extra : nullptr, n_docs, plan);
    rc = solve_pipeline(e, n_docs, pdx, e->d_bitmap.as<uint32_t>());
    if (rc) return rc;
    if (n_docs * words) {
        if (!hit_bitmap) return fail(e, GFT_E_INVALID, "null bitmap");
        HIP_TRY(hipMemcpyAsync(hit_bitmap, e->d_bitmap.p, n_docs * words * 4, hipMemcpyDeviceToHost, e->stream), "download");
    }
    HIP_TRY(hipStreamSynchronize(e->stream), "solve pipeline");
    return host_eval(e, pdx ? extra : nullptr, n_docs, plan, hit_bitmap, nullptr);
} GFT_CATCH((e ? &e->err : nullptr))

namespace {

// The three launches of the compaction on the engine's stream: popcount per row, the exclusive scan of the counts
// (k_scan_* of gft_kernels.hip), the fill.  fill == false: row_off only.  Nothing waits here.
int compact_enqueue(gft_engine* e, const uint32_t* d_bitmap, uint64_t n_docs, uint64_t* d_row_off, uint32_t* d_expr_idx,
                    uint32_t* d_label, uint64_t cap, bool count, bool fill) {
    hipStream_t st = e->stream;
    if (!n_docs || !e->n_exprs) {
        if (count) HIP_TRY(hipMemsetAsync(d_row_off, 0, (n_docs + 1) * 8, st), "row_off");
        return GFT_OK;
    }
    if (count) {
        HIP_TRY(e->sparse.cnt.ensure(n_docs * 4), "compact alloc");
        HIP_TRY(e->sparse.partial.ensure(scan_partials_needed(n_docs) * 8), "compact alloc");
        {
            ProfScope ps(e, "compact_count");
            HIP_TRY(launch_compact_count(d_bitmap, n_docs, e->n_exprs, e->sparse.cnt.as<uint32_t>(), e->n_cus, st), "compact count");
        }
        {
            ProfScope ps(e, "compact_scan");
            HIP_TRY(launch_exclusive_scan(e->sparse.cnt.as<uint32_t>(), n_docs, d_row_off, e->sparse.partial.as<uint64_t>(), st), "compact scan");
        }
    }
    if (fill && cap) {
        ProfScope ps(e, "compact_fill");
        HIP_TRY(launch_compact_fill(d_bitmap, n_docs, e->n_exprs, d_row_off, d_expr_idx, d_label, e->d_labels.as<uint32_t>(), cap,
                                    e->n_cus, st), "compact fill");
    }
    return GFT_OK;
}

// the CSR of a bitmap that is complete on the HOST (n_exprs columns) into the engine's result buffers
void sparse_from_host(gft_engine* e, const uint32_t* h_bitmap, uint64_t n_docs, gft_sparse* out) {
    e->sparse.h_row_off.assign(n_docs + 1, 0);
    const uint32_t* labels = e->have_labels ? e->h_labels.data() : nullptr;
    const uint64_t total = compact_host(h_bitmap, n_docs, e->n_exprs, labels, e->sparse.h_row_off.data(), nullptr, nullptr, 0);
    e->sparse.h_expr_idx.assign(total + 1, 0);
    e->sparse.h_label.assign(labels ? total + 1 : 1, 0);
    compact_host(h_bitmap, n_docs, e->n_exprs, labels, e->sparse.h_row_off.data(), e->sparse.h_expr_idx.data(), labels ? e->sparse.h_label.data() : nullptr, total);
    out->n_docs = n_docs; out->total = total;
    out->row_off = e->sparse.h_row_off.data(); out->expr_idx = e->sparse.h_expr_idx.data(); out->label = labels ? e->sparse.h_label.data() : nullptr;
}

// ... of a bitmap that is complete on the DEVICE: compacted there, only the CSR comes down (staged like every large result)
int sparse_from_device(gft_engine* e, const uint32_t* d_bitmap, uint64_t n_docs, gft_sparse* out) {
    HIP_TRY(e->sparse.row_off.ensure((n_docs + 1) * 8), "compact alloc");
    int rc = compact_enqueue(e, d_bitmap, n_docs, e->sparse.row_off.as<uint64_t>(), nullptr, nullptr, 0, true, false);
    if (rc) return rc;
    e->sparse.h_row_off.assign(n_docs + 1, 0);
    if ((rc = d2h_staged(e, e->sparse.h_row_off.data(), e->sparse.row_off.p, (n_docs + 1) * 8))) return rc;
    const uint64_t total = e->sparse.h_row_off[n_docs];
    const bool labels = e->have_labels;
    e->sparse.h_expr_idx.assign(total + 1, 0);
    e->sparse.h_label.assign(labels ? total + 1 : 1, 0);
    if (total) {
        HIP_TRY(e->sparse.idx.ensure(total * 4), "compact alloc");
        if (labels) HIP_TRY(e->sparse.label.ensure(total * 4), "compact alloc");
        rc = compact_enqueue(e, d_bitmap, n_docs, e->sparse.row_off.as<uint64_t>(), e->sparse.idx.as<uint32_t>(),
                             labels ? e->sparse.label.as<uint32_t>() : nullptr, total, false, true);
        if (rc) return rc;
        if ((rc = d2h_staged(e, e->sparse.h_expr_idx.data(), e->sparse.idx.p, total * 4))) return rc;
        if (labels && (rc = d2h_staged(e, e->sparse.h_label.data(), e->sparse.label.p, total * 4))) return rc;
    }
    out->n_docs = n_docs; out->total = total;
    out->row_off = e->sparse.h_row_off.data(); out->expr_idx = e->sparse.h_expr_idx.data(); out->label = labels ? e->sparse.h_label.data() : nullptr;
    return GFT_OK;
}

// gft_process, and gft_process_sparse (sparse != nullptr: the CSR instead of the rows) on one device
int process_host(gft_engine* e, const uint8_t* text_blob, const uint64_t* doc_off, uint64_t n_docs, uint32_t flags,
                 const gft_extra_matches* extra, uint32_t* hit_bitmap, gft_sparse* sparse) {
    if (int rc = check_ready(e, kNeedDevice | kNeedBuilt | kNeedPrograms | kNeedSettled)) return rc;
    DeviceGuard g(e->device);
    SyncOnExit drained(e);      // host buffers are read by asynchronous copies: drained on every way out
    // GFT_HOST_TIMING=1: where a call from host memory spends its time (stderr; tools/bench_latency.py)
    static const bool timing = getenv("GFT_HOST_TIMING") != nullptr;
    const auto t_begin = std::chrono::steady_clock::now();
    auto since = [&](const char* what) {
        if (!timing) return;
        (void)hipStreamSynchronize(e->stream);
        fprintf(stderr, "[gft host timing] %s: %.2f ms since the call began\n", what,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count());
    };
    int rc = stage_docs(e, text_blob, doc_off, n_docs);
    if (rc) return rc;
    since("text and offsets uploaded");
    gft_extra_matches dx;
    const gft_extra_matches* pdx = nullptr;
    rc = upload_extra(e, extra, n_docs, dx, pdx);
    if (rc) return rc;
    const uint64_t words = (e->n_exprs + 31) / 32;
    HIP_TRY(e->d_bitmap.ensure(std::max<uint64_t>(n_docs * words, 1) * 4), "bitmap alloc");
    HostPlan plan;                        // the (expression, document) pairs the host solves (normally none)
    plan_host(e, pdx ? extra : nullptr, n_docs, plan);
    BatchVerdict v;
    Publish publish{e, v};
    // (expressions beyond the device solver's limits need every match with its position: the scan then leaves the CSR too)
    rc = scan_pipeline(e, e->d_text.as<uint8_t>(), e->d_doc_off.as<uint64_t>(), n_docs, flags, plan.all_docs, v, doc_off);
    if (rc) return rc;
    e->pool.valid_docs = n_docs;          // gft_process_again may reuse this scan
    rc = solve_pipeline(e, n_docs, pdx, e->d_bitmap.as<uint32_t>());
    if (rc) return rc;
    if ((rc = refine_nonascii(e, e->d_text.as<uint8_t>(), e->d_doc_off.as<uint64_t>(), n_docs, flags, v))) return rc;
    since("scanned and solved");
    if (sparse && plan.empty()) {
        // the rows are complete where they are: compacted on the device, only the CSR comes down
        rc = sparse_from_device(e, e->d_bitmap.as<uint32_t>(), n_docs, sparse);
        since("compacted, lists downloaded");
        return rc;
    }
    if (sparse) {
        e->sparse.h_bitmap.assign(n_docs * words + 1, 0);
        hit_bitmap = e->sparse.h_bitmap.data();
    }
    if (n_docs * words) {
        if (!hit_bitmap) return fail(e, GFT_E_INVALID, "null bitmap");
        if ((rc = d2h_staged(e, hit_bitmap, e->d_bitmap.p, n_docs * words * 4))) return rc;
    }
    HIP_TRY(hipStreamSynchronize(e->stream), "process pipeline");
    since("bitmap downloaded");
    rc = host_eval(e, pdx ? extra : nullptr, n_docs, plan, hit_bitmap, nullptr);
    if (!rc && sparse) sparse_from_host(e, hit_bitmap, n_docs, sparse);
    return rc;
}

}  // namespace

int gft_process(gft_engine* e, const uint8_t* text_blob, const uint64_t* doc_off, uint64_t n_docs, uint32_t flags,
                const gft_extra_matches* extra, uint32_t* hit_bitmap) try {
    if (!e || (n_docs && !doc_off)) return e ? fail(e, GFT_E_INVALID, "null argument") : GFT_E_INVALID;
    GFT_LOCK(e);
    if (!e->peers.empty() && !e->in_multi && n_docs) return multi_process(e, text_blob, doc_off, n_docs, flags, extra, hit_bitmap);
    return process_host(e, text_blob, doc_off, n_docs, flags, extra, hit_bitmap, nullptr);
} GFT_CATCH((e ? &e->err : nullptr))

int gft_process_sparse(gft_engine* e, const uint8_t* text_blob, const uint64_t* doc_off, uint64_t n_docs, uint32_t flags,
                       const gft_extra_matches* extra, gft_sparse* out) try {
    if (!e || !out || (n_docs && !doc_off)) return e ? fail(e, GFT_E_INVALID, "null argument") : GFT_E_INVALID;
    GFT_LOCK(e);
    if (!e->peers.empty() && !e->in_multi && n_docs) {
        // (several devices: every shard's rows come to the host as they do for gft_process; sparse gathers are not built)
        e->sparse.h_bitmap.assign(n_docs * ((e->n_exprs + 31) / 32) + 1, 0);
        const int rc = multi_process(e, text_blob, doc_off, n_docs, flags, extra, e->sparse.h_bitmap.data());
        if (rc) return rc;
        sparse_from_host(e, e->sparse.h_bitmap.data(), n_docs, out);
        return GFT_OK;
    }
    return process_host(e, text_blob, doc_off, n_docs, flags, extra, nullptr, out);
} GFT_CATCH((e ? &e->err : nullptr))

int gft_compact_device(gft_engine* e, const uint32_t* d_hit_bitmap, uint64_t n_docs, uint64_t* d_row_off, uint32_t* d_expr_idx,
                       uint32_t* d_label, uint64_t cap, uint64_t* total) try {
    if (!e || !d_row_off) return e ? fail(e, GFT_E_INVALID, "null argument") : GFT_E_INVALID;
    GFT_LOCK(e);
    if (!e->peers.empty()) return fail(e, GFT_E_UNSUPPORTED, "gft_compact_device: single-device handles only (sparse gathers between devices are not built)");
    if (int rc = check_ready(e, kNeedDevice | kNeedPrograms)) return rc;
    if (n_docs && e->n_exprs && !d_hit_bitmap) return fail(e, GFT_E_INVALID, "null bitmap");
    if (cap && !d_expr_idx) return fail(e, GFT_E_INVALID, "gft_compact_device: cap entries but no expr_idx buffer");
    if (d_label && !e->have_labels) return fail(e, GFT_E_INVALID, "gft_compact_device: labels asked for, gft_set_expr_labels has not been called");
    if (total && !pend_settled(e))
        return fail(e, GFT_E_INVALID, "gft_compact_device: batches of gft_process_device_begin are in flight -- total must be NULL (the call must not wait)");
    DeviceGuard g(e->device);
    int rc = compact_enqueue(e, d_hit_bitmap, n_docs, d_row_off, d_expr_idx, d_label, cap, true, true);
    if (rc) return rc;
    if (total) {
        HIP_TRY(hipMemcpyAsync(total, d_row_off + n_docs, 8, hipMemcpyDeviceToHost, e->stream), "total read-back");
        HIP_TRY(hipStreamSynchronize(e->stream), "compaction");
    }
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

}  // extern "C"
