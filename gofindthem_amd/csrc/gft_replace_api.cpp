// gft_replace_api.cpp -- replace: every hit run rewritten by its replacement (gft_replace.hip, the run passes of gft_excerpt.hip):
// gft_replace_spans_device, and the host walk behind gft_debug_replace_spans.
#include <string.h>

#include <vector>

#include "gft_engine.hpp"
#include "gft_replace.hpp"
#include "gft_span_runs.hpp"

using namespace gft;
using namespace gft::api;

namespace {
constexpr RoomTexts kRepRoom{"no device memory for the replacement's work buffers", "replace alloc"};
const char kWho[] = "gft_replace_spans_device";
}  // namespace

extern "C" {

int gft_replace_spans_device(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs, const uint64_t* d_span_off,
                             const uint32_t* d_span_start, const uint32_t* d_span_len, const uint32_t* d_span_key, const uint32_t* key_rep,
                             uint32_t n_keys, const uint8_t* rep_bytes, const uint64_t* rep_off, uint32_t n_reps, uint32_t flags, uint8_t* d_out,
                             uint64_t cap_bytes, uint64_t* d_out_off, uint64_t* d_doc_run_off, uint32_t* d_run_new, uint32_t* d_run_len,
                             uint32_t* d_run_rep, uint64_t cap_runs, uint64_t* n_runs, uint64_t* total_bytes) try {
    if (!e) return GFT_E_INVALID;
    GFT_LOCK(e);
    if (n_runs) *n_runs = 0;
    if (total_bytes) *total_bytes = 0;
    if (flags) return fail(e, GFT_E_INVALID, std::string(kWho) + ": flags must be 0");
    if (!replace_table_ok(rep_bytes, rep_off, n_reps))
        return fail(e, GFT_E_INVALID, std::string(kWho) + ": the table has 1 .. 65536 replacements of GFT_REPLACE_MAX bytes at most, rep_off[0] == 0 "
                                                          "and ascending offsets");
    if (n_docs && (!d_doc_off || !d_span_off)) return fail(e, GFT_E_INVALID, "null argument");
    if (cap_bytes && !d_out) return fail(e, GFT_E_INVALID, std::string(kWho) + ": cap_bytes but no output buffer");
    if (cap_runs > (~0ull >> 4)) return fail(e, GFT_E_INVALID, std::string(kWho) + ": a size beyond the address space");
    if (!e->peers.empty()) return fail(e, GFT_E_UNSUPPORTED, std::string(kWho) + ": single-device handles only");
    int rc = check_ready(e, kNeedDevice | kNeedSettled, kWho);
    if (rc) return rc;
    if (n_docs > (~0ull >> 4)) return fail(e, GFT_E_INVALID, std::string(kWho) + ": a size beyond the address space");
    DeviceGuard g(e->device);
    hipStream_t st = e->stream;
    // the table and the key map are the caller's host memory: into vectors of this call's own (they outlive the drain)
    const uint32_t tab_bytes = (uint32_t)rep_off[n_reps];
    std::vector<uint8_t> h_tab((size_t)tab_bytes + 64, 0);
    if (tab_bytes) memcpy(h_tab.data(), rep_bytes, tab_bytes);
    const std::vector<uint64_t> h_off(rep_off, rep_off + n_reps + 1);
    std::vector<uint32_t> h_keys;
    if (d_span_key && key_rep) h_keys.assign(key_rep, key_rep + n_keys);
    // the run passes are the excerpt's, in the excerpt's buffers (gft_span_runs.hpp)
    auto& X = e->d_excerpt;
    auto& K = e->d_replace;
    SyncOnExit drain(e);                                            // (the pinned words and the vectors are handed to asynchronous copies)
    ReplaceParams P{};
    P.X.V = ExcView{d_text_blob, d_doc_off, n_docs, d_span_off, d_span_start, d_span_len, 0, 0, 0};
    SpanRun R{kWho, "replace", "heads", kRepRoom};
    if ((rc = span_run_begin(e, P.X, R))) return rc;
    const uint64_t n = R.n;
    if (replace_buffers_overlap(d_text_blob, R.lo, R.hi, d_doc_off, n_docs, d_span_off, d_span_start, d_span_len, d_span_key, R.s0, n, d_out,
                                cap_bytes, d_out_off, d_doc_run_off, d_run_new, d_run_len, d_run_rep, cap_runs))
        return fail(e, GFT_E_INVALID, std::string(kWho) + ": an output overlaps an input or another output");
    if ((rc = span_run_room(e, P.X, R, true)) || (rc = room(e, K.rid, n * 4, kRepRoom)) || (rc = room(e, K.pl, n * 4, kRepRoom)) ||
        (rc = room(e, K.ppos, (n + 1) * 8, kRepRoom)) || (rc = room(e, K.key_rep, h_keys.size() * 4, kRepRoom)) ||
        (rc = room(e, K.rep_off, h_off.size() * 8, kRepRoom)) || (rc = room(e, K.tab, h_tab.size(), kRepRoom)))
        return rc;
    P.span_key = d_span_key;
    P.key_rep = h_keys.empty() ? nullptr : K.key_rep.as<uint32_t>();
    P.n_keys = n_keys; P.n_reps = n_reps;
    P.rep_off = K.rep_off.as<uint64_t>(); P.tab = K.tab.as<uint8_t>(); P.tab_bytes = tab_bytes;
    P.rid = K.rid.as<uint32_t>(); P.pl = K.pl.as<uint32_t>(); P.ppos = K.ppos.as<uint64_t>();
    P.text_len = R.hi - R.lo;
    P.R.base = R.lo;
    if (d_span_key && key_rep && !n_keys && n) return fail(e, GFT_E_INVALID, std::string(kWho) + ": a key at or past n_keys (nothing was written)");
    HIP_TRY(hipMemcpyAsync(K.rep_off.p, h_off.data(), h_off.size() * 8, hipMemcpyHostToDevice, st), "replace table");
    HIP_TRY(hipMemcpyAsync(K.tab.p, h_tab.data(), h_tab.size(), hipMemcpyHostToDevice, st), "replace table");
    if (!h_keys.empty()) HIP_TRY(hipMemcpyAsync(K.key_rep.p, h_keys.data(), h_keys.size() * 4, hipMemcpyHostToDevice, st), "replace table");
    if ((rc = span_run_launch(e, P.X, R, "replace_runs", "replace_runs"))) return rc;
    {
        ProfScope ps(e, "replace_ids");
        if (n) {
            HIP_TRY(launch_exclusive_scan(P.X.head, n, X.rank.as<uint64_t>(), X.partial.as<uint64_t>(), st), "replace scan");
            HIP_TRY(hipMemsetAsync(K.rid.p, 0xFF, n * 4, st), "replace ids");
            HIP_TRY(launch_replace_ids(P, st), "replace ids kernel launch");
            HIP_TRY(launch_replace_len(P, st), "replace lengths kernel launch");
        }
    }
    {
        ProfScope ps(e, "replace_scan");
        if (n) {
            HIP_TRY(launch_exclusive_scan(P.X.share, n, X.pos.as<uint64_t>(), X.partial.as<uint64_t>(), st), "replace scan");
            HIP_TRY(launch_exclusive_scan(P.pl, n, K.ppos.as<uint64_t>(), X.partial.as<uint64_t>(), st), "replace scan");
        } else {                                                    // (no span: entry 0 is what the passes behind read)
            HIP_TRY(hipMemsetAsync(X.rank.p, 0, 8, st), "replace scan");
            HIP_TRY(hipMemsetAsync(X.pos.p, 0, 8, st), "replace scan");
            HIP_TRY(hipMemsetAsync(K.ppos.p, 0, 8, st), "replace scan");
        }
        HIP_TRY(launch_replace_check(P, st), "replace check kernel launch");
    }
    const uint64_t* h_ctl = X.pin;
    HIP_TRY(hipMemcpyAsync(X.pin, P.X.ctl, (kRepCtlKey + 1) * 8, hipMemcpyDeviceToHost, st), "replace totals");
    HIP_TRY(hipStreamSynchronize(st), "replace totals");
    if ((rc = span_run_verdict(e, R, h_ctl))) return rc;
    if (h_ctl[kRepCtlKey])
        return fail(e, GFT_E_INVALID, std::string(kWho) + ": a key at or past n_keys, or a replacement id at or past n_reps (nothing was written)");
    if (h_ctl[kRepCtlGrow])
        return fail(e, GFT_E_INVALID, std::string(kWho) + ": a document would reach 4 GiB once replaced (nothing was written)");
    const uint64_t runs = h_ctl[kExcCtlExc], total = n_docs ? h_ctl[kExcCtlTotal] : 0;
    if (n_runs) *n_runs = runs;
    if (total_bytes) *total_bytes = total;
    if ((rc = room(e, K.at, runs * 8, kRepRoom)) || (rc = room(e, K.delta, runs * 8, kRepRoom)) || (rc = room(e, K.len, runs * 4, kRepRoom)) ||
        (rc = room(e, K.roff, runs * 4, kRepRoom)))
        return rc;
    P.at = K.at.as<uint64_t>(); P.delta = K.delta.as<uint64_t>(); P.len = K.len.as<uint32_t>(); P.roff = K.roff.as<uint32_t>();
    P.R = RepPlan{P.at, P.delta, P.len, P.roff, runs, R.lo};
    P.out_off = d_out_off; P.doc_run_off = d_doc_run_off;
    P.run_new = d_run_new; P.run_len = d_run_len; P.run_rep = d_run_rep; P.cap_runs = cap_runs;
    P.out = d_out;
    P.G = sel_geom(total, cap_bytes, d_out);
    {
        ProfScope ps(e, "replace_place");
        HIP_TRY(launch_replace_place(P, st), "replace place kernel launch");
        if (!n_docs && d_out_off) HIP_TRY(hipMemsetAsync(d_out_off, 0, 8, st), "replace offsets");
        if (!n_docs && d_doc_run_off) HIP_TRY(hipMemsetAsync(d_doc_run_off, 0, 8, st), "replace offsets");
    }
    if (P.G.end) {
        ProfScope ps(e, "replace_copy");
        HIP_TRY(launch_replace_copy(P, st), "replace copy kernel launch");
    }
    HIP_TRY(hipStreamSynchronize(st), "replace copy");
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

int gft_debug_replace_spans(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const uint64_t* span_off, const uint32_t* span_start,
                            const uint32_t* span_len, const uint32_t* span_key, const uint32_t* key_rep, uint32_t n_keys, const uint8_t* rep_bytes,
                            const uint64_t* rep_off, uint32_t n_reps, uint32_t flags, uint8_t* out, uint64_t cap_bytes, uint64_t* out_off,
                            uint64_t* doc_run_off, uint32_t* run_new, uint32_t* run_len, uint32_t* run_rep, uint64_t cap_runs, uint64_t* n_runs,
                            uint64_t* total_bytes) try {
    return replace_spans_host(blob, doc_off, n_docs, span_off, span_start, span_len, span_key, key_rep, n_keys, rep_bytes, rep_off, n_reps, flags,
                              out, cap_bytes, out_off, doc_run_off, run_new, run_len, run_rep, cap_runs, n_runs, total_bytes);
} GFT_CATCH(nullptr)

void gft_debug_replace_shape(uint32_t* tile_spans, uint32_t* trip_tiles, uint32_t* chunk_bytes, uint32_t* tile_bytes, uint32_t* window,
                             uint32_t* lds_table) {
    if (tile_spans) *tile_spans = kExcTile;
    if (trip_tiles) *trip_tiles = kExcCarryTiles;
    if (chunk_bytes) *chunk_bytes = kSelChunk;
    if (tile_bytes) *tile_bytes = kSelTile;
    if (window) *window = kRepWindow;
    if (lds_table) *lds_table = kRepLdsTable;
}

}  // extern "C"
