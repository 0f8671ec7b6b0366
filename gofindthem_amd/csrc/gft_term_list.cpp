// gft_term_list.cpp -- the front end of the batch calls over a term list (batch_term_list: the refusals in their order, the four
// sources, the count-then-fill protocol of the kept list, the nonascii protocol) and the head of the calls that take such a list
// (list_head, list_check_launch, list_check_verdict).
#include "gft_term_list.hpp"

#include "gft_rank_piece.hpp"
#include "gft_words.hpp"

namespace gft::api {

int batch_term_list(gft_engine* e, const BatchList& A, TermList& out, int* nonascii) {
    out = TermList{nullptr, nullptr};
    if (nonascii) *nonascii = 0;
    const std::string w(A.who);
    if (A.n_docs && (!A.d_text || !A.d_doc_off)) return fail(e, GFT_E_INVALID, "null argument");
    if (A.flags & ~A.known_flags) return fail(e, GFT_E_INVALID, w + ": unknown flag bits");
    if (A.scan_flags & ~GFT_FOLD_ASCII) return fail(e, GFT_E_INVALID, w + ": scan_flags is GFT_FOLD_ASCII or 0");
    if (A.top && A.k > kRankMaxK) return fail(e, GFT_E_INVALID, w + ": k above 4096");
    if (A.top && A.k && (!A.d_top_idx || !A.d_top_score)) return fail(e, GFT_E_INVALID, "null argument");
    if (!e->peers.empty()) return fail(e, GFT_E_UNSUPPORTED, w + ": single-device handles only");
    int rc = check_ready(e, kNeedDevice);                           // (what else the handle must be, the source says under its own name)
    if (rc) return rc;
    if (A.n_docs > (A.words ? kWordsMax : ~0ull >> 4)) return fail(e, GFT_E_INVALID, w + ": a size beyond the address space");
    const bool may_leave = nonascii && (A.scan_flags & GFT_FOLD_ASCII) && A.n_docs;
    if (!A.d_hit_bitmap) {
        gft_matches m{};
        if ((rc = (A.words ? gft_scan_words_device : gft_scan_device)(e, A.d_text, A.d_doc_off, A.n_docs, A.scan_flags, &m))) return rc;
        if (may_leave && gft_last_nonascii(e)) { *nonascii = 1; return GFT_OK; }
        out = TermList{A.n_docs ? m.match_off : nullptr, m.term_id};
        return GFT_OK;
    }
    // the kept matches: counted, then filled into e->d_kept (the offsets are complete after the first call; the starts are what the
    // spans call asks for with any cap, and are not read)
    const auto spans = A.words ? gft_hit_spans_words_device : gft_hit_spans_device;
    auto& K = e->d_kept;
    uint64_t total = 0;
    {
        DeviceGuard g(e->device);
        if ((rc = room(e, K.off, (A.n_docs + 1) * 8, A.room))) return rc;
    }
    uint64_t* const off = K.off.as<uint64_t>();
    if ((rc = spans(e, A.d_text, A.d_doc_off, A.n_docs, A.scan_flags, A.d_hit_bitmap, nullptr, A.want, off, nullptr, nullptr, nullptr, 0, &total)))
        return rc;
    if (may_leave && gft_last_nonascii(e)) { *nonascii = 1; return GFT_OK; }
    if (total) {
        {
            DeviceGuard g(e->device);
            if ((rc = room(e, K.term, total * 4, A.room)) || (rc = room(e, K.start, total * 4, A.room))) return rc;
        }
        if ((rc = spans(e, A.d_text, A.d_doc_off, A.n_docs, A.scan_flags, A.d_hit_bitmap, nullptr, A.want, off, K.start.as<uint32_t>(), nullptr,
                        K.term.as<uint32_t>(), total, &total)))
            return rc;
    }
    out = TermList{A.n_docs ? off : nullptr, K.term.as<uint32_t>()};
    return GFT_OK;
}

int list_head(gft_engine* e, const char* who, const uint64_t* d_off, const uint32_t* d_term, uint64_t n_docs, uint32_t n_terms, ListEnds& L) {
    hipStream_t st = e->stream;
    uint64_t ends[2] = {0, 0};
    if (n_docs) {
        HIP_TRY(hipMemcpyAsync(&ends[0], d_off, 8, hipMemcpyDeviceToHost, st), "list offsets");
        HIP_TRY(hipMemcpyAsync(&ends[1], d_off + n_docs, 8, hipMemcpyDeviceToHost, st), "list offsets");
        HIP_TRY(hipStreamSynchronize(st), "list offsets");
    }
    if (ends[1] < ends[0]) return fail(e, GFT_E_INVALID, std::string(who) + ": offsets descend (nothing was written)");
    L = ListEnds{ends[0], ends[1] - ends[0]};
    if (L.n > (~0ull >> 4)) return fail(e, GFT_E_INVALID, std::string(who) + ": a size beyond the address space");
    if (L.n && !d_term) return fail(e, GFT_E_INVALID, "null argument");
    if (L.n && !n_terms) return fail(e, GFT_E_INVALID, std::string(who) + ": entries but no terms");
    return GFT_OK;
}

int list_check_launch(gft_engine* e, const char* stage, const uint64_t* d_off, const uint32_t* d_term, uint64_t n_docs, const ListEnds& L,
                      uint32_t n_terms, uint64_t* ctl) {
    const std::string s(stage);
    ProfScope ps(e, (s + "_check").c_str());
    StatsParams C{};                                                // (the check reads the list and writes the flag words)
    C.off = d_off; C.term = d_term; C.n_docs = n_docs; C.e0 = L.e0; C.n = L.n; C.n_terms = n_terms; C.ctl = ctl;
    HIP_TRY(launch_stats_check(C, e->n_cus, e->stream), (s + " check kernel launch").c_str());
    return GFT_OK;
}

int list_check_verdict(gft_engine* e, const char* who, const uint64_t* h_ctl, const char* indexed) {
    if (h_ctl[kStatsCtlOffs]) return fail(e, GFT_E_INVALID, std::string(who) + ": offsets descend (nothing was written)");
    if (h_ctl[kStatsCtlTerms])
        return fail(e, GFT_E_INVALID, std::string(who) + ": a term id that is no index of " + indexed + " (nothing was written)");
    return GFT_OK;
}

}  // namespace gft::api
