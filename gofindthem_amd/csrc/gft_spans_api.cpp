// gft_spans_api.cpp -- hit spans and redaction (gft_spans.hip): gft_hit_spans_device, gft_redact_spans_device, the lazy witness
// table, and the host walks behind gft_debug_witness_terms / gft_debug_hit_spans / gft_debug_redact_spans.
#include "gft_engine.hpp"
#include "gft_spans.hpp"
#include "witness_terms.hpp"

using namespace gft;
using namespace gft::api;

namespace {
constexpr RoomTexts kSpanRoom{"no device memory for the spans' work buffers", "spans alloc"};

// the witness table of the installed programs on the device: compiled and uploaded by the first call after a gft_set_programs
int ensure_witness_table(gft_engine* e) {
    auto& S = e->d_spans;
    if (S.wit_ready) return GFT_OK;
    WitnessTable tab;
    const uint32_t n_terms = (uint32_t)e->tables.tab.terms.size();
    if (compile_witness_terms(e->progs.prog.data(), e->progs.prog_off.data(), e->n_exprs, n_terms, n_terms + e->n_extra, tab))
        return fail(e, GFT_E_INTERNAL, "gft_hit_spans_device: the installed programs do not compile into a witness table");
    SyncOnExit drained(e);                                          // (the uploads read from `tab`)
    int rc;
    if ((rc = upload(e, S.wit_off, tab.off, "witness table upload")) || (rc = upload(e, S.wit_expr, tab.expr, "witness table upload"))) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream), "witness table upload");
    S.wit_ready = true;
    return GFT_OK;
}
}  // namespace

extern "C" {

int gft_hit_spans_device(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint32_t flags,
                         const uint32_t* d_hit_bitmap, const uint64_t* d_row_idx, const uint32_t* want, uint64_t* d_span_off,
                         uint32_t* d_span_start, uint32_t* d_span_len, uint32_t* d_span_term, uint64_t cap, uint64_t* total) try {
    if (!e) return GFT_E_INVALID;
    GFT_LOCK(e);
    if (total) *total = 0;
    if (n_docs && (!d_text_blob || !d_doc_off)) return fail(e, GFT_E_INVALID, "null argument");
    if (flags & ~GFT_FOLD_ASCII) return fail(e, GFT_E_INVALID, "gft_hit_spans_device: GFT_FOLD_ASCII is the only flag (spans are byte positions of every occurrence)");
    if (cap && !d_span_start) return fail(e, GFT_E_INVALID, "gft_hit_spans_device: cap entries but no span_start buffer");
    if (!e->peers.empty()) return fail(e, GFT_E_UNSUPPORTED, "gft_hit_spans_device: single-device handles only");
    int rc = check_ready(e, kNeedDevice | kNeedBuilt | kNeedPrograms | kNeedSettled, "gft_hit_spans_device");
    if (rc) return rc;
    const uint32_t W = (e->n_exprs + 31) / 32;
    if (n_docs && W && !d_hit_bitmap) return fail(e, GFT_E_INVALID, "null bitmap");
    if (cap > (~0ull >> 4) || n_docs > (~0ull >> 4)) return fail(e, GFT_E_INVALID, "gft_hit_spans_device: a size beyond the address space");
    DeviceGuard g(e->device);
    hipStream_t st = e->stream;
    if ((rc = ensure_witness_table(e))) return rc;
    // the scan, as gft_scan_device runs it: positions, the canonical CSR, the verdict
    BatchVerdict v;
    Publish publish{e, v};
    if ((rc = scan_pipeline(e, d_text_blob, d_doc_off, n_docs, flags, true, v))) return rc;
    if ((rc = refine_nonascii(e, d_text_blob, d_doc_off, n_docs, flags, v))) return rc;
    const uint64_t nm = v.total;
    {
        // (with d_row_idx the rows the call reads are not known on the host: the first row stands for the bitmap)
        const ByteRange ins[4] = {{d_text_blob ? d_text_blob + v.text_lo : nullptr, v.text_hi > v.text_lo ? v.text_hi - v.text_lo : 0},
                                  {d_doc_off, (n_docs + 1) * 8}, {d_hit_bitmap, (d_row_idx ? 1 : n_docs) * (uint64_t)W * 4}, {d_row_idx, n_docs * 8}};
        if (spans_outputs_overlap(d_span_off, n_docs, d_span_start, d_span_len, d_span_term, cap, ins, 4))
            return fail(e, GFT_E_INVALID, "gft_hit_spans_device: an output overlaps an input or another output");
    }
    if (!n_docs || !nm) {
        if (d_span_off) HIP_TRY(hipMemsetAsync(d_span_off, 0, (n_docs + 1) * 8, st), "span offsets");
        HIP_TRY(hipStreamSynchronize(st), "span offsets");
        return GFT_OK;
    }
    auto& S = e->d_spans;
    std::vector<uint32_t> h_want(std::max<uint32_t>(W, 1), 0);
    SyncOnExit drain(e);                                            // (h_want is handed to an asynchronous copy)
    if ((rc = room(e, S.want, (uint64_t)W * 4, kSpanRoom)) || (rc = room(e, S.keep, nm * 4, kSpanRoom)) ||
        (rc = room(e, S.rank, (nm + 1) * 8, kSpanRoom)) || (rc = room(e, S.partial, scan_partials_needed(nm) * 8, kSpanRoom)))
        return rc;
    SpanParams P{};
    P.match_off = e->d_match_off.as<uint64_t>(); P.term = e->d_term.as<uint32_t>(); P.pos = e->d_pos.as<uint32_t>();
    P.n_docs = n_docs; P.n_matches = nm;
    P.term_len = e->d_tabs.dfa.term_len.as<uint32_t>(); P.pos_end = (e->build_flags & GFT_POS_END) ? 1u : 0u;
    P.wit_off = S.wit_off.as<uint64_t>(); P.wit_expr = S.wit_expr.as<uint32_t>();
    P.bitmap = d_hit_bitmap; P.W = W; P.row_idx = d_row_idx;
    P.want = want ? S.want.as<uint32_t>() : nullptr;
    P.keep = S.keep.as<uint32_t>(); P.rank = S.rank.as<uint64_t>();
    P.span_off = d_span_off; P.span_start = d_span_start; P.span_len = d_span_len; P.span_term = d_span_term; P.cap = cap;
    {
        ProfScope ps(e, "span_mark");
        if (want && W) {
            for (uint32_t j = 0; j < W; j++) h_want[j] = want[j];
            HIP_TRY(hipMemcpyAsync(S.want.p, h_want.data(), (size_t)W * 4, hipMemcpyHostToDevice, st), "spans mask upload");
        }
        HIP_TRY(launch_span_mark(P, e->n_cus, st), "span mark kernel launch");
    }
    {
        ProfScope ps(e, "span_scan");
        HIP_TRY(launch_exclusive_scan(P.keep, nm, S.rank.as<uint64_t>(), S.partial.as<uint64_t>(), st), "span scan");
    }
    {
        ProfScope ps(e, "span_place");
        HIP_TRY(launch_span_place(P, st), "span place kernel launch");
    }
    uint64_t h_total = 0;
    HIP_TRY(hipMemcpyAsync(&h_total, P.rank + nm, 8, hipMemcpyDeviceToHost, st), "span total");
    HIP_TRY(hipStreamSynchronize(st), "span place");
    if (total) *total = h_total;
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

int gft_redact_spans_device(gft_engine* e, uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs, const uint64_t* d_span_off,
                            const uint32_t* d_span_start, const uint32_t* d_span_len, uint32_t mask_byte) try {
    if (!e) return GFT_E_INVALID;
    GFT_LOCK(e);
    if (mask_byte > 255) return fail(e, GFT_E_INVALID, "gft_redact_spans_device: the mask is one byte");
    if (n_docs && (!d_doc_off || !d_span_off)) return fail(e, GFT_E_INVALID, "null argument");
    if (!e->peers.empty()) return fail(e, GFT_E_UNSUPPORTED, "gft_redact_spans_device: single-device handles only");
    int rc = check_ready(e, kNeedDevice | kNeedSettled, "gft_redact_spans_device");
    if (rc) return rc;
    if (n_docs > (~0ull >> 4)) return fail(e, GFT_E_INVALID, "gft_redact_spans_device: a size beyond the address space");
    if (!n_docs) return GFT_OK;
    DeviceGuard g(e->device);
    hipStream_t st = e->stream;
    uint64_t ends[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(&ends[0], d_span_off, 8, hipMemcpyDeviceToHost, st), "span offsets");
    HIP_TRY(hipMemcpyAsync(&ends[1], d_span_off + n_docs, 8, hipMemcpyDeviceToHost, st), "span offsets");
    HIP_TRY(hipStreamSynchronize(st), "span offsets");
    if (ends[1] < ends[0] || ends[1] - ends[0] > (~0ull >> 4)) return fail(e, GFT_E_INVALID, "gft_redact_spans_device: span offsets descend");
    const uint64_t n = ends[1] - ends[0];
    if (!n) return GFT_OK;
    if (!d_text_blob || !d_span_start || !d_span_len) return fail(e, GFT_E_INVALID, "null argument");
    auto& S = e->d_spans;
    if ((rc = room(e, S.dst, n * 8, kSpanRoom)) || (rc = room(e, S.ctl, 4, kSpanRoom))) return rc;
    RedactParams P{};
    P.text = d_text_blob; P.doc_off = d_doc_off; P.n_docs = n_docs; P.span_off = d_span_off; P.span_start = d_span_start; P.span_len = d_span_len;
    P.s0 = ends[0]; P.n_spans = n; P.dst = S.dst.as<uint64_t>(); P.ctl = S.ctl.as<uint32_t>(); P.mask = mask_byte;
    {
        ProfScope ps(e, "redact_fill");
        HIP_TRY(hipMemsetAsync(P.ctl, 0, 4, st), "redact check");
        HIP_TRY(launch_redact_check(P, st), "redact check kernel launch");
        HIP_TRY(launch_redact_fill(P, st), "redact fill kernel launch");
    }
    uint32_t h_ctl = 0;
    HIP_TRY(hipMemcpyAsync(&h_ctl, P.ctl, 4, hipMemcpyDeviceToHost, st), "redact flag");
    HIP_TRY(hipStreamSynchronize(st), "redact fill");
    if (h_ctl) return fail(e, GFT_E_INVALID, "gft_redact_spans_device: a span reaches past the end of its document (nothing was written)");
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

int gft_debug_witness_terms(const uint32_t* prog_words, const uint64_t* prog_off, uint32_t n_exprs, uint32_t n_terms, uint32_t n_slots,
                            uint64_t* off, uint32_t* expr, uint64_t cap, uint64_t* needed) try {
    if (needed) *needed = 0;
    if (cap && !expr) return GFT_E_INVALID;
    WitnessTable tab;
    if (int rc = compile_witness_terms(prog_words, prog_off, n_exprs, n_terms, n_slots, tab)) return rc;
    if (needed) *needed = tab.expr.size();
    if (off) std::copy(tab.off.begin(), tab.off.end(), off);
    for (uint64_t k = 0; k < std::min<uint64_t>(cap, tab.expr.size()); k++) expr[k] = tab.expr[k];
    return GFT_OK;
} GFT_CATCH(nullptr)

int gft_debug_hit_spans(const uint64_t* match_off, const uint32_t* term_id, const uint32_t* pos, uint64_t n_docs, const uint32_t* term_len,
                        uint32_t pos_end, const uint64_t* wit_off, const uint32_t* wit_expr, const uint32_t* bitmap, uint32_t n_exprs,
                        const uint64_t* row_idx, const uint32_t* want, uint64_t* span_off, uint32_t* span_start, uint32_t* span_len,
                        uint32_t* span_term, uint64_t cap, uint64_t* total) try {
    return hit_spans_host(match_off, term_id, pos, n_docs, term_len, pos_end, wit_off, wit_expr, bitmap, n_exprs, row_idx, want, span_off,
                          span_start, span_len, span_term, cap, total);
} GFT_CATCH(nullptr)

int gft_debug_redact_spans(uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const uint64_t* span_off, const uint32_t* span_start,
                           const uint32_t* span_len, uint32_t mask_byte) try {
    return redact_spans_host(blob, doc_off, n_docs, span_off, span_start, span_len, mask_byte);
} GFT_CATCH(nullptr)

void gft_debug_spans_shape(uint32_t* tile_matches, uint32_t* tile_spans) {
    if (tile_matches) *tile_matches = kSpanMarkBlock;
    if (tile_spans) *tile_spans = kSpanTile;
}

}  // extern "C"
