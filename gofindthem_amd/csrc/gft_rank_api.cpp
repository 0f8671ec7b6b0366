// gft_rank_api.cpp -- a score per document, the k best documents and documents gathered by an index list (gft_rank.hip):
// gft_score_docs_device, gft_top_docs_device, gft_gather_docs_device, gft_batch_top_docs_device, and the host walks behind
// gft_debug_score_docs, gft_debug_top_docs and gft_debug_gather_docs.
#include "gft_doc_gather.hpp"
#include "gft_rank.hpp"
#include "gft_stats.hpp"
#include "gft_term_list.hpp"

using namespace gft;
using namespace gft::api;

namespace {
constexpr RoomTexts kRankRoom{"no device memory for the ranking's work buffers", "rank alloc"};
const char kWhoScore[] = "gft_score_docs_device";
const char kWhoTop[] = "gft_top_docs_device";
const char kWhoGather[] = "gft_gather_docs_device";
const char kWhoBatch[] = "gft_batch_top_docs_device";

// the workgroups of the score pass that are resident at a time (60 KB of LDS a workgroup: two on a compute unit)
uint32_t score_resident(unsigned n_cus) { return std::max(n_cus, 1u) * 2u; }

// gft_score_docs_device behind the handle's lock; max_out: the largest score (host)
int score_run(gft_engine* e, const char* who, const uint64_t* d_off, const uint32_t* d_term, uint64_t n_docs, uint32_t n_terms,
              const uint32_t* weights, uint32_t flags, uint64_t* d_score, uint64_t* max_out) {
    if (flags & ~GFT_SCORE_DISTINCT) return fail(e, GFT_E_INVALID, std::string(who) + ": unknown flag bits");
    if (n_docs && (!d_off || !d_score)) return fail(e, GFT_E_INVALID, "null argument");
    if (!e->peers.empty()) return fail(e, GFT_E_UNSUPPORTED, std::string(who) + ": single-device handles only");
    int rc = check_ready(e, kNeedDevice | kNeedSettled, who);
    if (rc) return rc;
    if (n_docs > (~0ull >> 4)) return fail(e, GFT_E_INVALID, std::string(who) + ": a size beyond the address space");
    DeviceGuard g(e->device);
    hipStream_t st = e->stream;
    SyncOnExit drain(e);                                            // (the weights and words of this frame are handed to asynchronous copies)
    ListEnds L{};
    if ((rc = list_head(e, who, d_off, d_term, n_docs, n_terms, L))) return rc;
    const uint64_t n = L.n;
    if (score_buffers_overlap(d_off, n_docs, d_term, L.e0, n, d_score)) return fail(e, GFT_E_INVALID, std::string(who) + ": the scores overlap an input");
    auto& R = e->d_rank;
    ScoreParams P{};
    P.off = d_off; P.term = d_term; P.n_docs = n_docs; P.e0 = L.e0; P.n = n; P.n_terms = n_terms;
    P.distinct = flags & GFT_SCORE_DISTINCT; P.score = d_score;
    P.grid = (uint32_t)stats_grid(n, n_docs, score_resident(e->n_cus));
    if ((rc = room(e, R.ctl, kRankCtlWords * 8, kRankRoom))) return rc;
    P.ctl = R.ctl.as<uint64_t>();
    if (weights && n_terms) {
        if ((rc = room(e, R.weights, (uint64_t)n_terms * 4, kRankRoom))) return rc;
        HIP_TRY(hipMemcpyAsync(R.weights.p, weights, (size_t)n_terms * 4, hipMemcpyHostToDevice, st), "score weights");
        P.weights = R.weights.as<uint32_t>();
    }
    if (P.distinct && n && !stats_bitset_in_lds(n_terms)) {
        const uint64_t bytes = (uint64_t)P.grid * stats_bitset_words(n_terms) * 4;
        if ((rc = room(e, R.rows, bytes, kRankRoom))) return rc;
        P.rows = R.rows.as<uint32_t>();
        HIP_TRY(hipMemsetAsync(P.rows, 0, bytes, st), "score bitset rows");
    }
    HIP_TRY(hipMemsetAsync(P.ctl, 0, kRankCtlWords * 8, st), "score control block");
    if ((rc = list_check_launch(e, "score", d_off, d_term, n_docs, L, n_terms, P.ctl))) return rc;
    {
        ProfScope ps(e, "score_docs");
        HIP_TRY(launch_score_docs(P, st), "score kernel launch");
    }
    uint64_t h_ctl[kRankCtlWords] = {0};
    HIP_TRY(hipMemcpyAsync(h_ctl, P.ctl, sizeof h_ctl, hipMemcpyDeviceToHost, st), "score flags");
    HIP_TRY(hipStreamSynchronize(st), "score flags");
    if ((rc = list_check_verdict(e, who, h_ctl, "the weights"))) return rc;
    if (max_out) *max_out = h_ctl[kRankCtlMax];
    return GFT_OK;
}

// gft_top_docs_device behind the handle's lock; known_max: NULL, or the largest score as the caller knows it
int top_run(gft_engine* e, const char* who, const uint64_t* d_score, uint64_t n_docs, uint32_t k, uint64_t doc_base, uint64_t* d_top_idx,
            uint64_t* d_top_score, uint64_t* n_top, const uint64_t* known_max) {
    if (n_top) *n_top = 0;
    if (k > kRankMaxK) return fail(e, GFT_E_INVALID, std::string(who) + ": k above 4096");
    if ((n_docs && !d_score) || (k && (!d_top_idx || !d_top_score))) return fail(e, GFT_E_INVALID, "null argument");
    if (!e->peers.empty()) return fail(e, GFT_E_UNSUPPORTED, std::string(who) + ": single-device handles only");
    int rc = check_ready(e, kNeedDevice | kNeedSettled, who);
    if (rc) return rc;
    if (n_docs > (~0ull >> 4)) return fail(e, GFT_E_INVALID, std::string(who) + ": a size beyond the address space");
    if (top_buffers_overlap(d_score, n_docs, k, d_top_idx, d_top_score))
        return fail(e, GFT_E_INVALID, std::string(who) + ": an output overlaps the scores or the other output");
    DeviceGuard g(e->device);
    hipStream_t st = e->stream;
    SyncOnExit drain(e);                                            // (words of this frame are handed to asynchronous copies)
    if (!k || !n_docs) return GFT_OK;
    auto& R = e->d_rank;
    TopParams P{};
    P.score = d_score; P.n_docs = n_docs; P.n_tiles = (n_docs + kRankPlaceTile - 1) / kRankPlaceTile; P.k = k; P.doc_base = doc_base;
    P.top_idx = d_top_idx; P.top_score = d_top_score;
    const uint64_t hist_bytes = (uint64_t)kRankMaxPasses * kRankBins * 8;
    if ((rc = room(e, R.ctl, kRankCtlWords * 8, kRankRoom)) || (rc = room(e, R.hist, hist_bytes, kRankRoom)) ||
        (rc = room(e, R.tile_gt, P.n_tiles * 4, kRankRoom)) || (rc = room(e, R.tile_eq, P.n_tiles * 4, kRankRoom)) ||
        (rc = room(e, R.gt_pos, (P.n_tiles + 1) * 8, kRankRoom)) || (rc = room(e, R.eq_pos, (P.n_tiles + 1) * 8, kRankRoom)) ||
        (rc = room(e, R.partial, scan_partials_needed(P.n_tiles) * 8, kRankRoom)) || (rc = room(e, R.cand_score, (uint64_t)k * 8, kRankRoom)) ||
        (rc = room(e, R.cand_idx, (uint64_t)k * 8, kRankRoom)))
        return rc;
    P.ctl = R.ctl.as<uint64_t>(); P.hist = R.hist.as<uint64_t>(); P.tile_gt = R.tile_gt.as<uint32_t>(); P.tile_eq = R.tile_eq.as<uint32_t>();
    P.gt_pos = R.gt_pos.as<uint64_t>(); P.eq_pos = R.eq_pos.as<uint64_t>(); P.cand_score = R.cand_score.as<uint64_t>(); P.cand_idx = R.cand_idx.as<uint64_t>();
    HIP_TRY(hipMemsetAsync(P.ctl, 0, kRankCtlWords * 8, st), "top control block");
    uint64_t mx = known_max ? *known_max : 0;
    if (!known_max) {
        {
            ProfScope ps(e, "top_max");
            HIP_TRY(launch_top_max(P, e->n_cus, st), "top max kernel launch");
        }
        HIP_TRY(hipMemcpyAsync(&mx, P.ctl + kRankCtlMax, 8, hipMemcpyDeviceToHost, st), "top max");
        HIP_TRY(hipStreamSynchronize(st), "top max");
    }
    if (!mx) return GFT_OK;                                         // no score above 0: nothing is listed
    const uint64_t krem = k;
    if (n_docs >= k) {
        // the k-th largest score exists: the select finds it (with fewer documents than k the threshold is 0, as the block holds it)
        ProfScope ps(e, "top_select");
        HIP_TRY(hipMemsetAsync(P.hist, 0, hist_bytes, st), "top histograms");
        HIP_TRY(hipMemcpyAsync(P.ctl + kRankCtlKrem, &krem, 8, hipMemcpyHostToDevice, st), "top rank");
        for (uint32_t p = rank_passes(mx); p--;) {
            P.shift = p * kRankDigitBits;
            HIP_TRY(launch_top_hist(P, e->n_cus, st), "top histogram kernel launch");
            HIP_TRY(launch_top_pick(P, st), "top pick kernel launch");
        }
    }
    {
        ProfScope ps(e, "top_place");
        HIP_TRY(launch_top_count(P, st), "top count kernel launch");
        HIP_TRY(launch_exclusive_scan(P.tile_gt, P.n_tiles, R.gt_pos.as<uint64_t>(), R.partial.as<uint64_t>(), st), "top scan");
        HIP_TRY(launch_exclusive_scan(P.tile_eq, P.n_tiles, R.eq_pos.as<uint64_t>(), R.partial.as<uint64_t>(), st), "top scan");
        HIP_TRY(launch_top_place(P, st), "top place kernel launch");
    }
    {
        ProfScope ps(e, "top_sort");
        HIP_TRY(launch_top_sort(P, st), "top sort kernel launch");
    }
    uint64_t listed = 0;
    HIP_TRY(hipMemcpyAsync(&listed, P.ctl + kRankCtlNTop, 8, hipMemcpyDeviceToHost, st), "top count");
    HIP_TRY(hipStreamSynchronize(st), "top count");
    if (n_top) *n_top = listed;
    return GFT_OK;
}

}  // namespace

namespace gft::api {

int batch_top_tail(gft_engine* e, const char* who, const uint64_t* d_off, const uint32_t* d_term, uint64_t n_docs, uint32_t n_terms,
                   const uint32_t* weights, uint32_t flags, uint32_t k, uint64_t doc_base, uint64_t* d_score, uint64_t* d_top_idx,
                   uint64_t* d_top_score, uint64_t* n_top) {
    int rc;
    if (!d_score && n_docs) {
        DeviceGuard g(e->device);
        if ((rc = room(e, e->d_rank.score, n_docs * 8, kRankRoom))) return rc;
        d_score = e->d_rank.score.as<uint64_t>();
    }
    if (top_buffers_overlap(d_score, n_docs, k, d_top_idx, d_top_score))
        return fail(e, GFT_E_INVALID, std::string(who) + ": an output overlaps the scores or the other output");
    uint64_t mx = 0;
    if ((rc = score_run(e, who, d_off, d_term, n_docs, n_terms, weights, flags, d_score, &mx))) return rc;
    return top_run(e, who, d_score, n_docs, k, doc_base, d_top_idx, d_top_score, n_top, &mx);
}

}  // namespace gft::api

extern "C" {

int gft_score_docs_device(gft_engine* e, const uint64_t* d_off, const uint32_t* d_term, uint64_t n_docs, uint32_t n_terms, const uint32_t* weights,
                          uint32_t flags, uint64_t* d_score, uint64_t* max_score) try {
    if (!e) return GFT_E_INVALID;
    GFT_LOCK(e);
    return score_run(e, kWhoScore, d_off, d_term, n_docs, n_terms, weights, flags, d_score, max_score);
} GFT_CATCH((e ? &e->err : nullptr))

int gft_top_docs_device(gft_engine* e, const uint64_t* d_score, uint64_t n_docs, uint32_t k, uint64_t doc_base, uint64_t* d_top_idx,
                        uint64_t* d_top_score, uint64_t* n_top) try {
    if (!e) return GFT_E_INVALID;
    GFT_LOCK(e);
    return top_run(e, kWhoTop, d_score, n_docs, k, doc_base, d_top_idx, d_top_score, n_top, nullptr);
} GFT_CATCH((e ? &e->err : nullptr))

int gft_gather_docs_device(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs, const uint64_t* d_idx, uint64_t m,
                           uint64_t idx_base, uint8_t* d_out, uint64_t cap_bytes, uint64_t* d_out_off, uint64_t* total_bytes) try {
    if (!e) return GFT_E_INVALID;
    GFT_LOCK(e);
    if (total_bytes) *total_bytes = 0;
    if (!d_out_off || (m && !d_idx) || (n_docs && (!d_doc_off || !d_text_blob))) return fail(e, GFT_E_INVALID, "null argument");
    if (cap_bytes && !d_out) return fail(e, GFT_E_INVALID, std::string(kWhoGather) + ": cap_bytes but no output buffer");
    if (!e->peers.empty()) return fail(e, GFT_E_UNSUPPORTED, std::string(kWhoGather) + ": single-device handles only");
    int rc = check_ready(e, kNeedDevice | kNeedSettled, kWhoGather);
    if (rc) return rc;
    if (m > (~0ull >> 4) || n_docs > (~0ull >> 4)) return fail(e, GFT_E_INVALID, std::string(kWhoGather) + ": a size beyond the address space");
    if (m && !n_docs) return fail(e, GFT_E_INVALID, std::string(kWhoGather) + ": an index that is no document of the batch (nothing was written)");
    constexpr DocGather kGather{kWhoGather, "gather", kRankRoom};
    DeviceGuard g(e->device);
    hipStream_t st = e->stream;
    if (!m) {
        if (ranges_meet(ByteRange{d_out_off, 8}, ByteRange{d_doc_off, (n_docs + 1) * 8})) return doc_gather_overlap(e, kGather);
        return doc_gather_empty(e, kGather, d_out_off);
    }
    auto& R = e->d_rank;
    if ((rc = room(e, R.ctl, kRankCtlWords * 8, kRankRoom)) || (rc = room(e, R.len, m * 4, kRankRoom)) || (rc = room(e, R.c_src, m * 8, kRankRoom)) ||
        (rc = room(e, R.c_off, (m + 1) * 8, kRankRoom)) || (rc = room(e, R.partial, scan_partials_needed(m) * 8, kRankRoom)))
        return rc;
    GatherParams P{d_doc_off, n_docs, d_idx, m, idx_base, R.len.as<uint32_t>(), R.c_src.as<uint64_t>(), R.ctl.as<uint64_t>()};
    uint64_t* const c_off = R.c_off.as<uint64_t>();
    HIP_TRY(hipMemsetAsync(P.ctl, 0, kRankCtlWords * 8, st), "gather control block");
    {
        ProfScope ps(e, "gather_place");
        HIP_TRY(launch_gather_place(P, e->n_cus, st), "gather place kernel launch");
    }
    {
        ProfScope ps(e, "gather_scan");
        HIP_TRY(launch_exclusive_scan(P.len, m, c_off, R.partial.as<uint64_t>(), st), "gather scan");
    }
    uint64_t h_ctl[kRankCtlWords] = {0}, total = 0;
    HIP_TRY(hipMemcpyAsync(h_ctl, P.ctl, sizeof h_ctl, hipMemcpyDeviceToHost, st), "gather totals");
    HIP_TRY(hipMemcpyAsync(&total, c_off + m, 8, hipMemcpyDeviceToHost, st), "gather totals");
    HIP_TRY(hipStreamSynchronize(st), "gather totals");
    if (h_ctl[kRankCtlBadIdx])
        return fail(e, GFT_E_INVALID, std::string(kWhoGather) + ": an index that is no document of the batch, offsets that descend, or a document of 4 GiB "
                                                                  "or more (nothing was written)");
    if (gather_buffers_overlap(d_text_blob, h_ctl[kRankCtlLo], h_ctl[kRankCtlHi], d_doc_off, n_docs, d_idx, m, d_out, cap_bytes, d_out_off))
        return doc_gather_overlap(e, kGather);
    if (total_bytes) *total_bytes = total;
    HIP_TRY(hipMemcpyAsync(d_out_off, c_off, (m + 1) * 8, hipMemcpyDeviceToDevice, st), "gather offsets");
    return doc_gather_copy(e, kGather, d_text_blob, c_off, P.c_src, m, total, d_out, cap_bytes);
} GFT_CATCH((e ? &e->err : nullptr))

int gft_batch_top_docs_device(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint32_t scan_flags,
                              const uint32_t* d_hit_bitmap, const uint32_t* want, const uint32_t* weights, uint32_t flags, uint32_t k,
                              uint64_t doc_base, uint64_t* d_score, uint64_t* d_top_idx, uint64_t* d_top_score, uint64_t* n_top,
                              int* nonascii) try {
    if (!e) return GFT_E_INVALID;
    GFT_LOCK(e);
    if (n_top) *n_top = 0;
    BatchList A{};
    A.who = kWhoBatch; A.d_text = d_text_blob; A.d_doc_off = d_doc_off; A.n_docs = n_docs; A.scan_flags = scan_flags;
    A.d_hit_bitmap = d_hit_bitmap; A.want = want; A.flags = flags; A.known_flags = GFT_SCORE_DISTINCT; A.room = kRankRoom;
    A.top = true; A.k = k; A.d_top_idx = d_top_idx; A.d_top_score = d_top_score;
    TermList T{};
    int rc = batch_term_list(e, A, T, nonascii);
    if (rc || (nonascii && *nonascii)) return rc;
    return batch_top_tail(e, kWhoBatch, T.off, T.term, n_docs, gft_n_terms(e), weights, flags, k, doc_base, d_score, d_top_idx, d_top_score, n_top);
} GFT_CATCH((e ? &e->err : nullptr))

int gft_debug_score_docs(const uint64_t* off, const uint32_t* term, uint64_t n_docs, uint32_t n_terms, const uint32_t* weights, uint32_t flags,
                         uint64_t* score, uint64_t* max_score) try {
    return score_docs_host(off, term, n_docs, n_terms, weights, flags, score, max_score);
} GFT_CATCH(nullptr)

int gft_debug_top_docs(const uint64_t* score, uint64_t n_docs, uint32_t k, uint64_t doc_base, uint64_t* top_idx, uint64_t* top_score,
                       uint64_t* n_top) try {
    return top_docs_host(score, n_docs, k, doc_base, top_idx, top_score, n_top);
} GFT_CATCH(nullptr)

int gft_debug_gather_docs(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const uint64_t* idx, uint64_t m, uint64_t idx_base,
                          uint8_t* out, uint64_t cap_bytes, uint64_t* out_off, uint64_t* total_bytes) try {
    return gather_docs_host(blob, doc_off, n_docs, idx, m, idx_base, out, cap_bytes, out_off, total_bytes);
} GFT_CATCH(nullptr)

void gft_debug_rank_shape(uint32_t* step_entries, uint32_t* step_docs, uint32_t* large_entries, uint32_t* set_slots, uint32_t* weight_lds_terms,
                          uint32_t* bitset_lds_terms, uint32_t* range_weight, uint32_t* digit_bits, uint32_t* place_tile, uint32_t* max_k) {
    if (step_entries) *step_entries = kStatsStep;
    if (step_docs) *step_docs = kStatsStepDocs;
    if (large_entries) *large_entries = kStatsLarge;
    if (set_slots) *set_slots = kStatsSetSlots;
    if (weight_lds_terms) *weight_lds_terms = kRankWeightLdsTerms;
    if (bitset_lds_terms) *bitset_lds_terms = kStatsBitsetLdsTerms;
    if (range_weight) *range_weight = kStatsRangeWeight;
    if (digit_bits) *digit_bits = kRankDigitBits;
    if (place_tile) *place_tile = kRankPlaceTile;
    if (max_k) *max_k = kRankMaxK;
}

}  // extern "C"
