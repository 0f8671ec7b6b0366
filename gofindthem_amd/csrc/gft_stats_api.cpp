// gft_stats_api.cpp -- term statistics of a match or span list and column counts of a hit bitmap (gft_stats.hip):
// gft_term_stats_device, gft_count_columns_device, gft_batch_term_stats_device, and the host walks behind gft_debug_term_stats and
// gft_debug_count_columns.
#include "gft_engine.hpp"
#include "gft_stats.hpp"
#include "gft_term_list.hpp"

using namespace gft;
using namespace gft::api;

namespace {
constexpr RoomTexts kStatsRoom{"no device memory for the statistics' work buffers", "stats alloc"};
const char kWho[] = "gft_term_stats_device";
const char kWhoCols[] = "gft_count_columns_device";
const char kWhoBatch[] = "gft_batch_term_stats_device";
}  // namespace

extern "C" {

int gft_term_stats_device(gft_engine* e, const uint64_t* d_off, const uint32_t* d_term, uint64_t n_docs, uint32_t n_terms, uint32_t flags,
                          uint64_t doc_base, uint64_t* d_occ, uint64_t* d_docs, uint64_t* d_first) try {
    if (!e) return GFT_E_INVALID;
    GFT_LOCK(e);
    if (flags & ~GFT_STATS_ACCUMULATE) return fail(e, GFT_E_INVALID, std::string(kWho) + ": unknown flag bits");
    if (n_docs && !d_off) return fail(e, GFT_E_INVALID, "null argument");
    if (!e->peers.empty()) return fail(e, GFT_E_UNSUPPORTED, std::string(kWho) + ": single-device handles only");
    int rc = check_ready(e, kNeedDevice | kNeedSettled, kWho);
    if (rc) return rc;
    if (n_docs > (~0ull >> 4)) return fail(e, GFT_E_INVALID, std::string(kWho) + ": a size beyond the address space");
    DeviceGuard g(e->device);
    hipStream_t st = e->stream;
    SyncOnExit drain(e);                                            // (words of this frame are handed to asynchronous copies)
    ListEnds L{};
    if ((rc = list_head(e, kWho, d_off, d_term, n_docs, n_terms, L))) return rc;
    const uint64_t n = L.n;
    if (stats_buffers_overlap(d_off, n_docs, d_term, L.e0, n, n_terms, d_occ, d_docs, d_first))
        return fail(e, GFT_E_INVALID, std::string(kWho) + ": an output overlaps an input or another output");
    auto& S = e->d_stats;
    StatsParams P{};
    P.off = d_off; P.term = d_term; P.n_docs = n_docs; P.e0 = L.e0; P.n = n; P.n_terms = n_terms;
    P.accumulate = flags & GFT_STATS_ACCUMULATE; P.doc_base = doc_base;
    P.occ = d_occ; P.docs = d_docs; P.first = d_first;
    P.grid = (uint32_t)stats_grid(n, n_docs, stats_resident(e->n_cus));
    const bool any_out = d_occ || d_docs || d_first;
    if ((rc = room(e, S.ctl, kStatsCtlWords * 8, kStatsRoom))) return rc;
    P.ctl = S.ctl.as<uint64_t>();
    if (any_out && n && !stats_bitset_in_lds(n_terms)) {
        const uint64_t bytes = (uint64_t)P.grid * stats_bitset_words(n_terms) * 4;
        if ((rc = room(e, S.rows, bytes, kStatsRoom))) return rc;
        P.rows = S.rows.as<uint32_t>();
        HIP_TRY(hipMemsetAsync(P.rows, 0, bytes, st), "stats bitset rows");
    }
    HIP_TRY(hipMemsetAsync(P.ctl, 0, kStatsCtlWords * 8, st), "stats control block");
    if ((rc = list_check_launch(e, "stats", d_off, d_term, n_docs, L, n_terms, P.ctl))) return rc;
    if (any_out) {
        ProfScope ps(e, "stats_count");
        if (!P.accumulate) HIP_TRY(launch_stats_init(P, st), "stats init kernel launch");
        HIP_TRY(launch_stats_count(P, st), "stats count kernel launch");
    }
    uint64_t h_ctl[kStatsCtlWords] = {0, 0};
    HIP_TRY(hipMemcpyAsync(h_ctl, P.ctl, sizeof h_ctl, hipMemcpyDeviceToHost, st), "stats flags");
    HIP_TRY(hipStreamSynchronize(st), "stats flags");
    return list_check_verdict(e, kWho, h_ctl, "the counters");
} GFT_CATCH((e ? &e->err : nullptr))

int gft_count_columns_device(gft_engine* e, const uint32_t* d_bitmap, uint64_t n_rows, uint32_t n_cols, const uint64_t* d_row_idx, uint32_t flags,
                             uint64_t* d_count) try {
    if (!e) return GFT_E_INVALID;
    GFT_LOCK(e);
    if (flags & ~GFT_STATS_ACCUMULATE) return fail(e, GFT_E_INVALID, std::string(kWhoCols) + ": unknown flag bits");
    if ((n_cols && !d_count) || (n_rows && n_cols && !d_bitmap)) return fail(e, GFT_E_INVALID, "null argument");
    if (!e->peers.empty()) return fail(e, GFT_E_UNSUPPORTED, std::string(kWhoCols) + ": single-device handles only");
    int rc = check_ready(e, kNeedDevice | kNeedSettled, kWhoCols);
    if (rc) return rc;
    const uint64_t groups = (n_rows + kStatsColRows - 1) / kStatsColRows;
    if (n_rows > (~0ull >> 4) || groups * std::max(stats_col_words(n_cols), 1u) >= (1ull << 31))
        return fail(e, GFT_E_INVALID, std::string(kWhoCols) + ": a size beyond the address space");
    if (columns_buffers_overlap(d_bitmap, n_rows, n_cols, d_row_idx, d_count))
        return fail(e, GFT_E_INVALID, std::string(kWhoCols) + ": the counts overlap an input");
    DeviceGuard g(e->device);
    hipStream_t st = e->stream;
    {
        ProfScope ps(e, "stats_columns");
        if (!(flags & GFT_STATS_ACCUMULATE) && n_cols) HIP_TRY(hipMemsetAsync(d_count, 0, (uint64_t)n_cols * 8, st), "column counts");
        HIP_TRY(launch_count_columns(ColumnParams{d_bitmap, d_row_idx, n_rows, n_cols, d_count}, st), "column count kernel launch");
    }
    HIP_TRY(hipStreamSynchronize(st), "column counts");
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

int gft_batch_term_stats_device(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint32_t scan_flags,
                                const uint32_t* d_hit_bitmap, const uint32_t* want, uint32_t flags, uint64_t doc_base, uint64_t* d_occ,
                                uint64_t* d_docs, uint64_t* d_first, int* nonascii) try {
    if (!e) return GFT_E_INVALID;
    GFT_LOCK(e);
    BatchList A{};
    A.who = kWhoBatch; A.d_text = d_text_blob; A.d_doc_off = d_doc_off; A.n_docs = n_docs; A.scan_flags = scan_flags;
    A.d_hit_bitmap = d_hit_bitmap; A.want = want; A.flags = flags; A.known_flags = GFT_STATS_ACCUMULATE; A.room = kStatsRoom;
    TermList T{};
    int rc = batch_term_list(e, A, T, nonascii);
    if (rc || (nonascii && *nonascii)) return rc;
    return gft_term_stats_device(e, T.off, T.term, n_docs, gft_n_terms(e), flags, doc_base, d_occ, d_docs, d_first);
} GFT_CATCH((e ? &e->err : nullptr))

int gft_debug_term_stats(const uint64_t* off, const uint32_t* term, uint64_t n_docs, uint32_t n_terms, uint32_t flags, uint64_t doc_base,
                         uint64_t* occ, uint64_t* docs, uint64_t* first) try {
    return term_stats_host(off, term, n_docs, n_terms, flags, doc_base, occ, docs, first);
} GFT_CATCH(nullptr)

int gft_debug_count_columns(const uint32_t* bitmap, uint64_t n_rows, uint32_t n_cols, const uint64_t* row_idx, uint32_t flags,
                            uint64_t* count) try {
    return count_columns_host(bitmap, n_rows, n_cols, row_idx, flags, count);
} GFT_CATCH(nullptr)

void gft_debug_stats_shape(uint32_t* step_entries, uint32_t* step_docs, uint32_t* set_slots, uint32_t* cache_slots, uint32_t* large_entries,
                           uint32_t* bitset_lds_terms, uint32_t* range_weight, uint32_t* column_rows) {
    if (step_entries) *step_entries = kStatsStep;
    if (step_docs) *step_docs = kStatsStepDocs;
    if (set_slots) *set_slots = kStatsSetSlots;
    if (cache_slots) *cache_slots = kStatsCacheSlots;
    if (large_entries) *large_entries = kStatsLarge;
    if (bitset_lds_terms) *bitset_lds_terms = kStatsBitsetLdsTerms;
    if (range_weight) *range_weight = kStatsRangeWeight;
    if (column_rows) *column_rows = kStatsColRows;
}

}  // extern "C"
