// gft_words_api.cpp -- whole-word matching (gft_words.hip): gft_filter_word_matches_device and what is built on it --
// gft_scan_words_device, gft_process_words_device / gft_process_words, gft_hit_spans_words_device,
// gft_batch_term_stats_words_device, gft_batch_top_docs_words_device -- and the host walk behind gft_debug_filter_word_matches.
#include "gft_engine.hpp"
#include "gft_term_list.hpp"
#include "gft_words.hpp"

using namespace gft;
using namespace gft::api;

namespace {
constexpr RoomTexts kWordsRoom{"no device memory for the word filter's work buffers", "words alloc"};
const char kWho[] = "gft_filter_word_matches_device";
const char kWhoScan[] = "gft_scan_words_device";
const char kWhoProcess[] = "gft_process_words_device";
const char kWhoSpans[] = "gft_hit_spans_words_device";
const char kWhoStats[] = "gft_batch_term_stats_words_device";
const char kWhoTop[] = "gft_batch_top_docs_words_device";
}  // namespace

// the class table on the device: uploaded by the first call of a handle (the excerpt's word snap asks for it too)
int gft::ensure_word_table(gft_engine* e) {
    auto& S = e->d_words;
    if (S.table_up) return GFT_OK;
    const WordTable& T = word_table_host();
    int rc;
    if ((rc = room(e, S.tab_row, kWordBlocks * 2, kWordsRoom)) || (rc = room(e, S.tab_bits, (uint64_t)word_table_rows() * 32, kWordsRoom))) return rc;
    HIP_TRY(hipMemcpyAsync(S.tab_row.p, T.row, kWordBlocks * 2, hipMemcpyHostToDevice, e->stream), "word table upload");
    HIP_TRY(hipMemcpyAsync(S.tab_bits.p, T.bits, (size_t)word_table_rows() * 32, hipMemcpyHostToDevice, e->stream), "word table upload");
    HIP_TRY(hipStreamSynchronize(e->stream), "word table upload");
    S.table_up = true;
    return GFT_OK;
}

namespace {

struct FilterArgs {
    const uint8_t* text; const uint64_t* doc_off; uint64_t n_docs;
    const uint64_t* off; const uint32_t* pos; const uint32_t* len; const uint32_t* term; const uint32_t* term_len;
    uint32_t n_terms, flags;
    uint64_t* out_off; uint32_t* out_pos; uint32_t* out_len; uint32_t* out_term; uint64_t cap;
    const void* more_in[2]; uint64_t more_n[2];                     // further inputs the outputs must not meet (nullable)
};

// the filter behind the lock and the handle's checks, under the caller's DeviceGuard; waits for the stream
int filter_run(gft_engine* e, const FilterArgs& A, uint64_t* total, const char* who) {
    if (total) *total = 0;
    hipStream_t st = e->stream;
    const std::string w(who);
    if (A.flags & ~GFT_WORDS_POS_END) return fail(e, GFT_E_INVALID, w + ": unknown flag bits");
    if (A.cap && !A.out_pos) return fail(e, GFT_E_INVALID, w + ": cap entries but no position buffer");
    if (A.n_docs && (!A.doc_off || !A.off)) return fail(e, GFT_E_INVALID, "null argument");
    if (A.n_docs > kWordsMax || A.cap > (~0ull >> 4)) return fail(e, GFT_E_INVALID, w + ": a size beyond the address space");
    if (!A.n_docs) {
        if (A.out_off) HIP_TRY(hipMemsetAsync(A.out_off, 0, 8, st), "list offsets");
        HIP_TRY(hipStreamSynchronize(st), "list offsets");
        return GFT_OK;
    }
    SyncOnExit drain(e);                                            // (words of this frame are handed to asynchronous copies)
    uint64_t ends[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(&ends[0], A.off, 8, hipMemcpyDeviceToHost, st), "list offsets");
    HIP_TRY(hipMemcpyAsync(&ends[1], A.off + A.n_docs, 8, hipMemcpyDeviceToHost, st), "list offsets");
    HIP_TRY(hipMemcpyAsync(&ends[2], A.doc_off, 8, hipMemcpyDeviceToHost, st), "document offsets");
    HIP_TRY(hipMemcpyAsync(&ends[3], A.doc_off + A.n_docs, 8, hipMemcpyDeviceToHost, st), "document offsets");
    HIP_TRY(hipStreamSynchronize(st), "list offsets");
    if (ends[1] < ends[0]) return fail(e, GFT_E_INVALID, w + ": offsets descend (nothing was written)");
    const uint64_t e0 = ends[0], n = ends[1] - ends[0];
    if (n > kWordsMax) return fail(e, GFT_E_INVALID, w + ": a size beyond the address space");
    if (n && (!A.text || !A.pos || (!A.len && (!A.term || !A.term_len)))) return fail(e, GFT_E_INVALID, "null argument");
    if (n && A.out_term && !A.term) return fail(e, GFT_E_INVALID, w + ": term ids asked for, none given");
    {
        const ByteRange ins[9] = {{A.text ? A.text + ends[2] : nullptr, ends[3] > ends[2] ? ends[3] - ends[2] : 0},
                                  {A.doc_off, (A.n_docs + 1) * 8}, {A.off, (A.n_docs + 1) * 8}, {A.pos ? A.pos + e0 : nullptr, n * 4},
                                  {A.len ? A.len + e0 : nullptr, n * 4}, {A.term ? A.term + e0 : nullptr, n * 4},
                                  {A.len ? nullptr : A.term_len, (uint64_t)A.n_terms * 4}, {A.more_in[0], A.more_n[0]}, {A.more_in[1], A.more_n[1]}};
        if (words_outputs_overlap(A.out_off, A.n_docs, A.out_pos, A.out_len, A.out_term, A.cap, ins, 9))
            return fail(e, GFT_E_INVALID, w + ": an output overlaps an input or another output");
    }
    auto& S = e->d_words;
    int rc;
    if ((rc = ensure_word_table(e))) return rc;
    if ((rc = room(e, S.ctl, kWordsCtlWords * 4, kWordsRoom)) || (rc = room(e, S.keep, n * 4, kWordsRoom)) ||
        (rc = room(e, S.rank, (n + 1) * 8, kWordsRoom)) || (rc = room(e, S.partial, scan_partials_needed(std::max<uint64_t>(n, 1)) * 8, kWordsRoom)))
        return rc;
    WordsParams P{};
    P.text = A.text; P.doc_off = A.doc_off; P.n_docs = A.n_docs; P.off = A.off; P.e0 = e0; P.n = n;
    P.pos = A.pos; P.len = A.len; P.term = A.term; P.term_len = A.term_len; P.n_terms = A.n_terms;
    P.pos_end = (A.flags & GFT_WORDS_POS_END) ? 1u : 0u;
    P.table = WordTable{S.tab_row.as<uint16_t>(), S.tab_bits.as<uint32_t>()};
    P.ctl = S.ctl.as<uint32_t>(); P.keep = S.keep.as<uint32_t>(); P.rank = S.rank.as<uint64_t>();
    P.out_off = A.out_off; P.out_pos = A.out_pos; P.out_len = A.out_len; P.out_term = A.out_term; P.cap = A.cap;
    HIP_TRY(hipMemsetAsync(P.ctl, 0, kWordsCtlWords * 4, st), "words control block");
    {
        ProfScope ps(e, "word_check");
        HIP_TRY(launch_words_check(P, e->n_cus, st), "word check kernel launch");
    }
    if (n) {
        {
            ProfScope ps(e, "word_mark");
            HIP_TRY(launch_words_mark(P, e->n_cus, st), "word mark kernel launch");
        }
        {
            ProfScope ps(e, "word_scan");
            HIP_TRY(launch_exclusive_scan(P.keep, n, S.rank.as<uint64_t>(), S.partial.as<uint64_t>(), st), "word scan");
        }
        {
            ProfScope ps(e, "word_place");
            HIP_TRY(launch_words_place(P, st), "word place kernel launch");
        }
    }
    uint32_t h_ctl[kWordsCtlWords] = {0, 0, 0, 0};
    uint64_t h_total = 0;
    HIP_TRY(hipMemcpyAsync(h_ctl, P.ctl, sizeof h_ctl, hipMemcpyDeviceToHost, st), "words flags");
    if (n) HIP_TRY(hipMemcpyAsync(&h_total, P.rank + n, 8, hipMemcpyDeviceToHost, st), "words total");
    HIP_TRY(hipStreamSynchronize(st), "word place");
    if (h_ctl[kWordsCtlOffs]) return fail(e, GFT_E_INVALID, w + ": offsets descend (nothing was written)");
    if (h_ctl[kWordsCtlTerms]) return fail(e, GFT_E_INVALID, w + ": a term id that is no index of the term lengths (nothing was written)");
    if (h_ctl[kWordsCtlRange]) return fail(e, GFT_E_INVALID, w + ": an entry reaches out of its document (nothing was written)");
    if (!n && A.out_off) {
        HIP_TRY(hipMemsetAsync(A.out_off, 0, (A.n_docs + 1) * 8, st), "list offsets");
        HIP_TRY(hipStreamSynchronize(st), "list offsets");
    }
    if (total) *total = h_total;
    return GFT_OK;
}

// the canonical CSR of the scan that just ran (nm matches) filtered into the engine's own list (d_words.off / pos / term)
int filter_scan(gft_engine* e, const uint8_t* d_text, const uint64_t* d_doc_off, uint64_t n_docs, uint64_t nm, uint64_t* kept, const char* who) {
    auto& S = e->d_words;
    int rc;
    if ((rc = room(e, S.off, (n_docs + 1) * 8, kWordsRoom)) || (rc = room(e, S.pos, nm * 4, kWordsRoom)) || (rc = room(e, S.term, nm * 4, kWordsRoom)))
        return rc;
    FilterArgs A{};
    A.text = d_text; A.doc_off = d_doc_off; A.n_docs = n_docs;
    A.off = e->d_match_off.as<uint64_t>(); A.pos = e->d_pos.as<uint32_t>(); A.term = e->d_term.as<uint32_t>();
    A.term_len = e->d_tabs.dfa.term_len.as<uint32_t>(); A.n_terms = (uint32_t)e->tables.tab.terms.size();
    A.flags = (e->build_flags & GFT_POS_END) ? GFT_WORDS_POS_END : 0u;
    A.out_off = S.off.as<uint64_t>(); A.out_pos = S.pos.as<uint32_t>(); A.out_term = S.term.as<uint32_t>(); A.cap = nm;
    return filter_run(e, A, kept, who);
}

// gft_process_words_device behind its lock and the handle's checks
int process_words_sync(gft_engine* e, const uint8_t* d_text, const uint64_t* d_doc_off, uint64_t n_docs, uint32_t flags, uint32_t* d_bitmap,
                       BatchVerdict& v) {
    if (flags & ~GFT_FOLD_ASCII) return fail(e, GFT_E_INVALID, std::string(kWhoProcess) + ": GFT_FOLD_ASCII is the only flag");
    if (!e->peers.empty()) return fail(e, GFT_E_UNSUPPORTED, std::string(kWhoProcess) + ": single-device handles only");
    int rc = check_ready(e, kNeedDevice | kNeedBuilt | kNeedPrograms | kNeedSettled, kWhoProcess);
    if (rc) return rc;
    if (!e->progs.host_only.empty())
        return fail(e, GFT_E_UNSUPPORTED, std::string(kWhoProcess) + ": an expression beyond the device solver's limits (gft_n_host_exprs) is not solved from whole-word matches");
    if (n_docs && e->n_exprs && !d_bitmap) return fail(e, GFT_E_INVALID, "null bitmap");
    DeviceGuard g(e->device);
    // the scan with positions and the canonical CSR, as gft_scan_device runs it
    if ((rc = scan_pipeline(e, d_text, d_doc_off, n_docs, flags, true, v))) return rc;
    if ((rc = refine_nonascii(e, d_text, d_doc_off, n_docs, flags, v))) return rc;
    if (!n_docs || !e->n_exprs) return GFT_OK;
    const uint64_t n_units = e->pool.n_units;
    uint64_t kept = 0;
    if ((rc = filter_scan(e, d_text, d_doc_off, n_docs, v.total, &kept, kWhoProcess))) return rc;
    // The solver reads a document's matches unit by unit and then the caller-supplied list: the units stay where they are (every
    // document has one) with nothing in them, the kept matches are the list (slot = term id).  What the unit table and the pool
    // hold is no scan any more: gft_process_again finds nothing to reuse.  (The solver takes a minimum over a slot's positions,
    // and the kept list is ascending per term anyway: no host read-back for INORD.)
    e->pool = PoolState();
    HIP_TRY(hipMemsetAsync(e->d_unit_count.p, 0, n_units * 4, e->stream), "unit counts");
    auto& S = e->d_words;
    const gft_extra_matches x{S.off.as<uint64_t>(), S.term.as<uint32_t>(), S.pos.as<uint32_t>()};
    if ((rc = solve_pipeline(e, n_docs, &x, d_bitmap))) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream), "process pipeline");
    return GFT_OK;
}
}  // namespace

extern "C" {

int gft_filter_word_matches_device(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs, const uint64_t* d_off,
                                   const uint32_t* d_pos, const uint32_t* d_len, const uint32_t* d_term, const uint32_t* d_term_len,
                                   uint32_t n_terms, uint32_t flags, uint64_t* d_out_off, uint32_t* d_out_pos, uint32_t* d_out_len,
                                   uint32_t* d_out_term, uint64_t cap, uint64_t* total) try {
    if (!e) return GFT_E_INVALID;
    GFT_LOCK(e);
    if (total) *total = 0;
    if (!e->peers.empty()) return fail(e, GFT_E_UNSUPPORTED, std::string(kWho) + ": single-device handles only");
    int rc = check_ready(e, kNeedDevice | kNeedSettled, kWho);
    if (rc) return rc;
    DeviceGuard g(e->device);
    FilterArgs A{};
    A.text = d_text_blob; A.doc_off = d_doc_off; A.n_docs = n_docs; A.off = d_off; A.pos = d_pos; A.len = d_len; A.term = d_term;
    A.term_len = d_term_len; A.n_terms = n_terms; A.flags = flags;
    A.out_off = d_out_off; A.out_pos = d_out_pos; A.out_len = d_out_len; A.out_term = d_out_term; A.cap = cap;
    return filter_run(e, A, total, kWho);
} GFT_CATCH((e ? &e->err : nullptr))

int gft_scan_words_device(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint32_t flags,
                          gft_matches* out_dev) try {
    if (!e || !out_dev || (n_docs && (!d_text_blob || !d_doc_off))) return e ? fail(e, GFT_E_INVALID, "null argument") : GFT_E_INVALID;
    GFT_LOCK(e);
    if (flags & ~GFT_FOLD_ASCII) return fail(e, GFT_E_INVALID, std::string(kWhoScan) + ": GFT_FOLD_ASCII is the only flag (whole words are judged at byte positions of every occurrence)");
    if (!e->peers.empty()) return fail(e, GFT_E_UNSUPPORTED, std::string(kWhoScan) + ": single-device handles only");
    int rc = check_ready(e, kNeedDevice | kNeedBuilt | kNeedSettled, kWhoScan);
    if (rc) return rc;
    DeviceGuard g(e->device);
    BatchVerdict v;
    Publish publish{e, v};
    if ((rc = scan_pipeline(e, d_text_blob, d_doc_off, n_docs, flags, true, v))) return rc;
    if ((rc = refine_nonascii(e, d_text_blob, d_doc_off, n_docs, flags, v))) return rc;
    uint64_t kept = 0;
    if ((rc = filter_scan(e, d_text_blob, d_doc_off, n_docs, v.total, &kept, kWhoScan))) return rc;
    out_dev->n_docs = n_docs; out_dev->n_matches = kept;
    out_dev->match_off = e->d_words.off.as<uint64_t>();
    out_dev->term_id = e->d_words.term.as<uint32_t>();
    out_dev->pos = e->d_words.pos.as<uint32_t>();
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

int gft_process_words_device(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint32_t flags,
                             uint32_t* d_hit_bitmap) try {
    if (!e || (n_docs && (!d_text_blob || !d_doc_off))) return e ? fail(e, GFT_E_INVALID, "null argument") : GFT_E_INVALID;
    GFT_LOCK(e);
    BatchVerdict v;
    Publish publish{e, v};
    return process_words_sync(e, d_text_blob, d_doc_off, n_docs, flags, d_hit_bitmap, v);
} GFT_CATCH((e ? &e->err : nullptr))

int gft_process_words(gft_engine* e, const uint8_t* text_blob, const uint64_t* doc_off, uint64_t n_docs, uint32_t flags,
                      uint32_t* hit_bitmap) try {
    if (!e || (n_docs && !doc_off)) return e ? fail(e, GFT_E_INVALID, "null argument") : GFT_E_INVALID;
    GFT_LOCK(e);
    if (!e->peers.empty()) return fail(e, GFT_E_UNSUPPORTED, "gft_process_words: single-device handles only");
    int rc = check_ready(e, kNeedDevice | kNeedBuilt | kNeedPrograms | kNeedSettled, "gft_process_words");
    if (rc) return rc;
    const uint64_t words = (e->n_exprs + 31) / 32;
    if (n_docs * words && !hit_bitmap) return fail(e, GFT_E_INVALID, "null bitmap");
    DeviceGuard g(e->device);
    SyncOnExit drained(e);                                          // host buffers are read by asynchronous copies: drained on every way out
    if ((rc = stage_docs(e, text_blob, doc_off, n_docs))) return rc;
    HIP_TRY(e->d_bitmap.ensure(std::max<uint64_t>(n_docs * words, 1) * 4), "bitmap alloc");
    BatchVerdict v;
    Publish publish{e, v};
    if ((rc = process_words_sync(e, e->d_text.as<uint8_t>(), e->d_doc_off.as<uint64_t>(), n_docs, flags, e->d_bitmap.as<uint32_t>(), v))) return rc;
    if (n_docs * words && (rc = d2h_staged(e, hit_bitmap, e->d_bitmap.p, n_docs * words * 4))) return rc;
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

int gft_hit_spans_words_device(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint32_t flags,
                               const uint32_t* d_hit_bitmap, const uint64_t* d_row_idx, const uint32_t* want, uint64_t* d_span_off,
                               uint32_t* d_span_start, uint32_t* d_span_len, uint32_t* d_span_term, uint64_t cap, uint64_t* total) try {
    if (!e) return GFT_E_INVALID;
    GFT_LOCK(e);
    if (total) *total = 0;
    if (cap && !d_span_start) return fail(e, GFT_E_INVALID, std::string(kWhoSpans) + ": cap entries but no span_start buffer");
    if (cap > (~0ull >> 4) || n_docs > kWordsMax) return fail(e, GFT_E_INVALID, std::string(kWhoSpans) + ": a size beyond the address space");
    // the call's spans, counted and then filled into buffers of the engine's (the offsets are complete after the first call)
    auto& S = e->d_words;
    uint64_t n_spans = 0;
    int rc;
    {
        DeviceGuard g(e->device);
        if (e->device >= 0 && (rc = room(e, S.span_off, (n_docs + 1) * 8, kWordsRoom))) return rc;
    }
    if ((rc = gft_hit_spans_device(e, d_text_blob, d_doc_off, n_docs, flags, d_hit_bitmap, d_row_idx, want, S.span_off.as<uint64_t>(), nullptr, nullptr,
                                   nullptr, 0, &n_spans)))
        return rc;
    {
        DeviceGuard g(e->device);
        if ((rc = room(e, S.span_start, n_spans * 4, kWordsRoom)) || (rc = room(e, S.span_len, n_spans * 4, kWordsRoom)) ||
            (rc = room(e, S.span_term, n_spans * 4, kWordsRoom)))
            return rc;
    }
    if (n_spans) {
        if ((rc = gft_hit_spans_device(e, d_text_blob, d_doc_off, n_docs, flags, d_hit_bitmap, d_row_idx, want, S.span_off.as<uint64_t>(),
                                       S.span_start.as<uint32_t>(), S.span_len.as<uint32_t>(), S.span_term.as<uint32_t>(), n_spans, &n_spans)))
            return rc;
    }
    DeviceGuard g(e->device);
    const uint32_t W = (e->n_exprs + 31) / 32;
    FilterArgs A{};
    A.text = d_text_blob; A.doc_off = d_doc_off; A.n_docs = n_docs;
    A.off = S.span_off.as<uint64_t>(); A.pos = S.span_start.as<uint32_t>(); A.len = S.span_len.as<uint32_t>(); A.term = S.span_term.as<uint32_t>();
    A.out_off = d_span_off; A.out_pos = d_span_start; A.out_len = d_span_len; A.out_term = d_span_term; A.cap = cap;
    // (with d_row_idx the rows the call reads are not known on the host: the first row stands for the bitmap)
    A.more_in[0] = d_hit_bitmap; A.more_n[0] = (d_row_idx ? 1 : n_docs) * (uint64_t)W * 4;
    A.more_in[1] = d_row_idx; A.more_n[1] = n_docs * 8;
    return filter_run(e, A, total, kWhoSpans);
} GFT_CATCH((e ? &e->err : nullptr))

int gft_batch_term_stats_words_device(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint32_t scan_flags,
                                      const uint32_t* d_hit_bitmap, const uint32_t* want, uint32_t flags, uint64_t doc_base, uint64_t* d_occ,
                                      uint64_t* d_docs, uint64_t* d_first, int* nonascii) try {
    if (!e) return GFT_E_INVALID;
    GFT_LOCK(e);
    BatchList A{};
    A.who = kWhoStats; A.words = true; A.d_text = d_text_blob; A.d_doc_off = d_doc_off; A.n_docs = n_docs; A.scan_flags = scan_flags;
    A.d_hit_bitmap = d_hit_bitmap; A.want = want; A.flags = flags; A.known_flags = GFT_STATS_ACCUMULATE; A.room = kWordsRoom;
    TermList T{};
    int rc = batch_term_list(e, A, T, nonascii);
    if (rc || (nonascii && *nonascii)) return rc;
    return gft_term_stats_device(e, T.off, T.term, n_docs, gft_n_terms(e), flags, doc_base, d_occ, d_docs, d_first);
} GFT_CATCH((e ? &e->err : nullptr))

int gft_batch_top_docs_words_device(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint32_t scan_flags,
                                    const uint32_t* d_hit_bitmap, const uint32_t* want, const uint32_t* weights, uint32_t flags, uint32_t k,
                                    uint64_t doc_base, uint64_t* d_score, uint64_t* d_top_idx, uint64_t* d_top_score, uint64_t* n_top,
                                    int* nonascii) try {
    if (!e) return GFT_E_INVALID;
    GFT_LOCK(e);
    if (n_top) *n_top = 0;
    BatchList A{};
    A.who = kWhoTop; A.words = true; A.d_text = d_text_blob; A.d_doc_off = d_doc_off; A.n_docs = n_docs; A.scan_flags = scan_flags;
    A.d_hit_bitmap = d_hit_bitmap; A.want = want; A.flags = flags; A.known_flags = GFT_SCORE_DISTINCT; A.room = kWordsRoom;
    A.top = true; A.k = k; A.d_top_idx = d_top_idx; A.d_top_score = d_top_score;
    TermList T{};
    int rc = batch_term_list(e, A, T, nonascii);
    if (rc || (nonascii && *nonascii)) return rc;
    return batch_top_tail(e, kWhoTop, T.off, T.term, n_docs, gft_n_terms(e), weights, flags, k, doc_base, d_score, d_top_idx, d_top_score, n_top);
} GFT_CATCH((e ? &e->err : nullptr))

int gft_debug_filter_word_matches(const uint8_t* text, const uint64_t* doc_off, uint64_t n_docs, const uint64_t* off, const uint32_t* pos,
                                  const uint32_t* len, const uint32_t* term, const uint32_t* term_len, uint32_t n_terms, uint32_t flags,
                                  uint64_t* out_off, uint32_t* out_pos, uint32_t* out_len, uint32_t* out_term, uint64_t cap, uint64_t* total) try {
    return filter_word_matches_host(text, doc_off, n_docs, off, pos, len, term, term_len, n_terms, flags, out_off, out_pos, out_len, out_term, cap,
                                    total);
} GFT_CATCH(nullptr)

uint32_t gft_debug_word_rune(uint32_t cp) { return words_is_word(word_table_host(), cp); }

void gft_debug_words_shape(uint32_t* tile_entries, uint32_t* table_rows, uint32_t* table_bytes) {
    if (tile_entries) *tile_entries = kWordsTile;
    if (table_rows) *table_rows = word_table_rows();
    if (table_bytes) *table_bytes = kWordBlocks * 2u + word_table_rows() * 32u;
}

}  // extern "C"
