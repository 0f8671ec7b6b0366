// gft_pipeline.cpp -- the kernel pipelines behind gft_scan* / gft_process*: the unit table, the scan launch with its retry,
// the verdict on a deferred launch, the unique / rune / solve pipelines and what the host solves.  Host orchestration only.
#include "gft_engine.hpp"

#include <cstdio>

#include "host_solve.hpp"

#ifndef GFT_EXTRA_KERNELS
// The earlier suffix-window kernels (gft_scan2.hip, gft_scan4.hip) are cross-checks and study objects: a product build
// does not carry them (python -m gofindthem_amd.build with GFT_EXTRA_KERNELS=1 does).  Without them nothing "fits".
namespace gft {
bool scan2_plan(uint32_t, uint32_t, uint32_t, uint32_t, size_t, uint32_t*, uint32_t*) { return false; }
hipError_t launch_scan2(const Scan2Params&, uint32_t, unsigned, hipStream_t) { return hipErrorNotSupported; }
bool scan4_plan(uint32_t, uint32_t, uint32_t, uint32_t, size_t, bool, uint32_t*, uint32_t*) { return false; }
hipError_t launch_scan4(const Scan2Params&, uint32_t, unsigned, hipStream_t) { return hipErrorNotSupported; }
}  // namespace gft
namespace gft::api { const bool kExtraKernels = false; }
#else
namespace gft::api { const bool kExtraKernels = true; }
#endif

namespace gft::api {

static int ensure_pool(gft_engine* e, uint64_t entries) {
    if (entries <= e->pool_cap) return GFT_OK;
    HIP_TRY(e->d_pool_term.ensure(entries * 4), "pool alloc");
    HIP_TRY(e->d_pool_pos.ensure(entries * 4), "pool alloc");
    e->pool_cap = std::min(e->d_pool_term.cap, e->d_pool_pos.cap) / 4;
    return GFT_OK;
}

// slabs of the last completed scan -> canonical CSR in e->d_match_off / d_term / d_pos (document order, the reference's
// emission order inside a document).  The unit table, the slabs and the counts of that scan are still in the engine
// (e->pool); positions must have been written (want_pos).
static int csr_from_pool(gft_engine* e, uint64_t n_docs) {
    hipStream_t st = e->stream;
    const uint64_t n_units = e->pool.n_units, total = e->pool.total;
    HIP_TRY(e->d_term.ensure(std::max<uint64_t>(total, 1) * 4), "result alloc");
    HIP_TRY(e->d_pos.ensure(std::max<uint64_t>(total, 1) * 4), "result alloc");
    HIP_TRY(e->d_unit_out.ensure((n_units + 1) * 8), "unit alloc");
    HIP_TRY(e->d_partial.ensure(scan_partials_needed(std::max(n_units, n_docs)) * 8), "unit alloc");
    ProfScope ps(e, "aux");
    HIP_TRY(launch_exclusive_scan(e->d_unit_count.as<uint32_t>(), n_units, e->d_unit_out.as<uint64_t>(),
                                  e->d_partial.as<uint64_t>(), st), "unit_out scan");
    // (the suffix-window kernels leave a unit's matches in any order -- shifted anchors report a term from another position
    // than its end, also on scan2's per-lane path: the gather sorts them)
    const bool sort_units = counts_slabs(e->plan.kernel);
    HIP_TRY(launch_gather(e->d_unit_start.as<uint64_t>(), e->d_unit_count.as<uint32_t>(),
                          e->d_unit_out.as<uint64_t>(), n_units, e->d_pool_term.as<uint32_t>(),
                          e->d_pool_pos.as<uint32_t>(), e->d_term.as<uint32_t>(), e->d_pos.as<uint32_t>(),
                          e->d_unit_base.as<uint64_t>(), n_docs, e->d_match_off.as<uint64_t>(), e->n_cus, st,
                          sort_units ? e->d_units.as<Unit>() : nullptr,
                          e->d_tabs.dfa.term_len.as<uint32_t>(), (e->build_flags & GFT_POS_END) ? 1u : 0u),
            "gather");
    e->pool.csr_valid = true;
    return GFT_OK;
}

// What varies from batch to batch in the parameters of a scan launch
struct ScanBatch {
    const uint8_t* d_text; const uint64_t* d_doc_off;
    uint64_t n_docs, n_units, text_hi;
    uint32_t flags, unit_max;
    bool need_csr;
};

// where the kernels and the copies find a field of the control block (byte offsets: batch_verdict.hpp)
template <class T>
T* ctl_at(const gft_engine* e, size_t byte_off) { return reinterpret_cast<T*>(e->d_ctl.as<uint8_t>() + byte_off); }

// the fields that every scan kernel's parameter struct has
template <class Params>
void fill_common(const gft_engine* e, const ScanBatch& b, Params& P) {
    P.text = b.d_text; P.doc_off = b.d_doc_off; P.units = e->d_units.as<Unit>(); P.n_units = b.n_units;
    P.pos_end = (e->build_flags & GFT_POS_END) ? 1 : 0;
    P.fold = (b.flags & GFT_FOLD_ASCII) ? 1 : 0;
    P.nonascii = ctl_at<uint32_t>(e, kCtlNonascii);
    P.cursor = ctl_at<uint64_t>(e, kCtlCursor); P.pool_cap = e->pool_cap;
    P.pool_term = e->d_pool_term.as<uint32_t>(); P.pool_pos = e->d_pool_pos.as<uint32_t>();
    P.unit_start = e->d_unit_start.as<uint64_t>(); P.unit_count = e->d_unit_count.as<uint32_t>();
}
// ... and those of the suffix-window kernels
template <class Params>
void fill_window(const gft_engine* e, const ScanBatch& b, Params& P) {
    fill_common(e, b, P);
    P.text_bytes = b.text_hi;
    P.n_matches = ctl_at<uint64_t>(e, kCtlTotal);
    // presence-only mode: positions are only read by INORD groups (and by CSR callers)
    P.want_pos = (b.need_csr || e->progs.n_inord_groups > 0) ? 1 : 0;
    // wave priorities: the latency-bound verification stages overtake the filter phase of the other waves (5 % on
    // the benchmark; GFT_SCAN_PRIO=0 switches it off)
    P.prio = e->opt_scan_prio;
    P.dbg = e->opt_scan_dbg;
}

// The waves of a launch over `work` items (units; chunks for scan4): every wave of the grid owns a slab from the start
static uint64_t grid_waves(const gft_engine* e, uint64_t work) {
    const uint64_t wpw = e->plan.scan_waves;
    return std::min<uint64_t>(std::max<uint64_t>((work + wpw - 1) / wpw, 1), e->n_cus) * wpw;
}
// the smallest slab of scan2 / scan3 / scan5 (scan4 sizes its slabs from a chunk's need)
constexpr uint64_t slab_floor(ScanKernel k) { return k == ScanKernel::scan3 ? 2 * kScan3MinRoom : 64; }
// ... and their slab: the slack is at most one slab per resident wave, keep it below half the pool
static uint32_t slab_size(const gft_engine* e) {
    const uint64_t n_waves = (uint64_t)e->n_cus * e->plan.scan_waves;
    return (uint32_t)std::min<uint64_t>(kScan2Slab, std::max<uint64_t>(slab_floor(e->plan.kernel), e->pool_cap / (2 * n_waves)));
}

static ScanParams dfa_params(const gft_engine* e, const ScanBatch& b) {
    ScanParams P;
    fill_common(e, b, P);
    const AcTables& tab = e->tables.tab;
    const auto& d = e->d_tabs.dfa;
    P.byte_class = d.byte_class.as<uint8_t>(); P.delta = d.delta.as<uint32_t>();
    P.out_term = d.out_term.as<uint32_t>(); P.out_link = d.out_link.as<uint32_t>();
    P.term_len = d.term_len.as<uint32_t>();
    P.n_classes = tab.n_classes; P.n_states = tab.n_states; P.n_lds_states = e->plan.n_lds_states;
    P.max_term_len = tab.max_term_len;
    return P;
}

static Scan3Params scan3_params(const gft_engine* e, const ScanBatch& b) {
    Scan3Params P;
    fill_window(e, b, P);
    const Scan3Tables& s3 = e->tables.s3;
    const auto& d = e->d_tabs.s3;
    P.cls = P.fold ? d.cls_fold.as<uint8_t>() : d.cls.as<uint8_t>();
    P.filter = d.filter.as<uint32_t>(); P.filter_words = (uint32_t)s3.filter.size();
    P.short3 = d.short3.as<uint8_t>(); P.short3_bytes = (uint32_t)s3.short3.size();
    P.srec = d.srec.as<uint32_t>(); P.srec_words = (uint32_t)s3.srec.size();
    P.short3_big = s3.short3_big.empty() ? nullptr : d.short3_big.as<uint32_t>();
    P.srec_big = d.srec_big.as<uint32_t>();
    P.bloom = d.bloom.as<uint32_t>(); P.bloom_lg = s3.bloom_lg; P.bloom_lds = s3.bloom_lg <= kScan3BloomLdsLg ? 1 : 0;
    P.slots = d.slots.as<Scan2Slot>(); P.slot_shift = s3.slot_shift; P.slot_seed = s3.slot_seed;
    P.more = d.more.as<Scan2Slot>();
    P.term_blob = d.term_blob.as<uint8_t>(); P.term_off = d.term_off.as<uint32_t>();
    P.G = s3.G; P.grouped = s3.grouped ? 1 : 0;
    P.cand_cap = e->plan.scan3_cand_cap;
    P.slab = slab_size(e);
    return P;
}

// scan2's parameters, with what scan4 / scan5 add to them when one of those is the engine's kernel
static Scan2Params scan2_params(const gft_engine* e, const ScanBatch& b) {
    Scan2Params P;
    fill_window(e, b, P);
    const Scan2Tables& s2 = e->tables.s2;
    const Scan3Tables& s3 = e->tables.s3;
    const gft_engine::TableBufs& d = e->d_tabs;
    P.filter = d.s2.filter.as<uint32_t>(); P.filter_words = (uint32_t)s2.filter.size();
    P.hashed = s2.hashed ? 1 : 0; P.hash_shift = s2.hash_shift;
    P.short3 = d.s2.short3.as<uint8_t>(); P.short3_bytes = (uint32_t)s2.short3.size();
    P.fpt = d.s2.fpt.as<uint8_t>(); P.fpt_lg = s2.fpt_lg;
    P.shorts_packed = d.s2.shorts_packed.as<uint32_t>(); P.shorts_words = (uint32_t)std::min<size_t>(s2.shorts_packed.size(), 255 * 3);
    P.short3_big = s2.short3_big.empty() ? nullptr : d.s2.short3_big.as<uint32_t>();
    P.cand_cap = e->plan.scan2_cand_cap;
    P.slots = d.s2.slots.as<Scan2Slot>(); P.slot_shift = s2.slot_shift; P.slot_seed = s2.slot_seed;
    P.more = d.s2.more.as<Scan2Slot>();
    P.cls = P.fold ? d.s2.cls_fold.as<uint8_t>() : d.s2.cls.as<uint8_t>();
    P.term_blob = d.s2.term_blob.as<uint8_t>(); P.term_off = d.s2.term_off.as<uint32_t>();
    P.kp = s2.kp; P.pad_class = s2.pad_class;
    // the balanced path serves both callers: the solver reads presence / successor positions in any order, and
    // CSR results are put into emission order by the gather (k_gather_sorted).  GFT_SCAN_ORDERED=1 sends every unit
    // through the kernel's per-lane staging path (normally the fallback for units whose matches overflow the LDS
    // fifo): a second implementation of the verification, kept as a cross-check
    P.ordered = (b.need_csr && e->opt_scan_ordered) ? 1 : 0;
    P.dbg_counters = (P.dbg & (2 | 64)) ? e->d_dbg.as<uint64_t>() : nullptr;
    P.slab = slab_size(e);
    if (e->plan.kernel == ScanKernel::scan4) {
        // the streaming form: chunks of up to eight units (fewer when the batch is small: every wave should get several
        // chunks), a fifo in place of the candidate list, per-unit regions sized from the density seen so far
        const uint64_t n_waves = (uint64_t)e->n_cus * e->plan.scan_waves;
        P.chunk_units = (uint32_t)std::min<uint64_t>(kScan4ChunkUnits, std::max<uint64_t>(1, b.n_docs / (n_waves * 4)));
        if (e->opt_scan4_chunk) P.chunk_units = std::min<uint32_t>(e->opt_scan4_chunk, kScan4ChunkUnits);      // (GFT_SCAN4_CHUNK: tests)
        P.cand_cap = e->plan.scan4_fifo[P.want_pos ? 1 : 0];
        P.bound_q16 = (uint32_t)std::min<double>(e->learned.scan4_density * 1.6 * 65536.0 + 1.0, 4.0e9);
        P.bound_add = 48;
        P.round_c = e->opt_scan4_round ? std::min<uint32_t>(64, std::max<uint32_t>(16, e->opt_scan4_round & ~15u)) : 64;   // (GFT_SCAN4_ROUND: timing studies)
        // a slab should hold a few chunks' regions (the rest of a slab that the next chunk does not fit is lost)
        const uint64_t chunk_need = (uint64_t)P.chunk_units * (((uint64_t)b.unit_max * P.bound_q16 >> 16) + P.bound_add);
        P.slab = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(kScan2Slab, 4 * chunk_need), std::max<uint64_t>(chunk_need, e->pool_cap / (2 * n_waves)));
    } else if (e->plan.kernel == ScanKernel::scan5) {
        // one filter probe per two bytes: scan2's tables behind the 3-gram filter over merged classes
        P.s5_filter = d.s5.filter.as<uint64_t>(); P.s5_dual = (uint32_t)e->s5.filter.size();
        P.s5_grp = P.fold ? d.s5.grp_fold.as<uint8_t>() : d.s5.grp.as<uint8_t>();
        P.s5_G = e->s5.G; P.s5_pad_g = e->s5.pad_group;
        P.s5_fifo_cap = e->plan.s5plan.fifo_cap; P.cand_cap = e->plan.s5plan.cand_cap;
        P.s5_sG = 0; P.s5_sgrp = nullptr; P.s5_srec_big = nullptr;
        if (e->plan.s5_short_groups) {
            // more than 32 byte classes: the short terms through the group-indexed tables of scan3's set
            P.short3 = d.s3.short3.as<uint8_t>(); P.short3_bytes = (uint32_t)s3.short3.size();
            P.shorts_packed = d.s3.srec.as<uint32_t>(); P.shorts_words = (uint32_t)s3.srec.size();
            P.short3_big = s3.short3_big.empty() ? nullptr : d.s3.short3_big.as<uint32_t>();
            P.s5_srec_big = d.s3.srec_big.as<uint32_t>();
            P.s5_sgrp = P.fold ? d.s3.cls_fold.as<uint8_t>() : d.s3.cls.as<uint8_t>();
            P.s5_sG = s3.G;
        }
        P.s5_term_bits = e->plan.s5_term_bits; P.s5_pos_bias = e->plan.s5_pos_bias;
        P.s5_bloom = e->plan.s5_bloom_lg ? d.s5.bloom.as<uint32_t>() : nullptr; P.s5_bloom_lg = e->plan.s5_bloom_lg;
    }
    return P;
}

// Puts the engine's scan kernel on the stream once, over the whole pool as it is now; L learns what the launch owned.
static int enqueue_scan(gft_engine* e, const ScanBatch& b, ScanLaunch& L) {
    hipStream_t st = e->stream;
    const ScanKernel k = e->plan.kernel;
    ScanParams Pd; Scan3Params P3; Scan2Params P2;
    uint64_t work = b.n_units, slab = 0;
    L.ordered = false;
    if (k == ScanKernel::dfa) Pd = dfa_params(e, b);
    else if (k == ScanKernel::scan3) { P3 = scan3_params(e, b); slab = P3.slab; }
    else {
        if (e->opt_scan_dbg & (2 | 64)) {
            HIP_TRY(e->d_dbg.ensure(128), "debug alloc");
            HIP_TRY(hipMemsetAsync(e->d_dbg.p, 0, 128, st), "memset");
        }
        P2 = scan2_params(e, b); slab = P2.slab;
        L.ordered = P2.ordered != 0;
        if (k == ScanKernel::scan4) work = (b.n_units + P2.chunk_units - 1) / P2.chunk_units;
    }
    // every wave of the grid owns one slab from the start; the cursor counts what is taken behind those (the DFA kernel's
    // counts matches: nothing is owned)
    L.static_slabs = counts_slabs(k) ? grid_waves(e, work) * slab : 0;
    {
        ProfScope ps(e, "scan");
        HIP_TRY(k == ScanKernel::dfa     ? launch_scan_units(Pd, e->n_cus, st)
                : k == ScanKernel::scan2 ? launch_scan2(P2, e->plan.scan_waves, e->n_cus, st)
                : k == ScanKernel::scan3 ? launch_scan3(P3, e->plan.scan_waves, e->n_cus, st)
                : k == ScanKernel::scan4 ? launch_scan4(P2, e->plan.scan_waves, e->n_cus, st)
                                         : launch_scan5(P2, e->n_cus, st), "scan kernel launch");
    }
    if (on_scan2_tables(k) && (e->opt_scan_dbg & 64)) {
        // phase clocks: a wave's cycles per unit (0 first bytes, 1 filter, 2 candidate list, 3 stage A, 4 stage B, 5 flush,
        // 7 unit record), averaged over all units
        const uint64_t n_units = b.n_units;
        uint64_t t[16];
        HIP_TRY(hipMemcpyAsync(t, e->d_dbg.p, sizeof t, hipMemcpyDeviceToHost, st), "debug read-back");
        HIP_TRY(hipStreamSynchronize(st), "debug read-back");
        if (k == ScanKernel::scan5) fprintf(stderr, "[gft scan debug] scan5 (G=%u, list %u):\n", e->s5.G, e->plan.s5plan.cand_cap);
        if (k == ScanKernel::scan4)
            fprintf(stderr, "[gft scan debug] scan4 wave cycles per unit: chunk set-up %.0f, filter %.0f, queue push %.0f, stage A issue %.0f, stage A %.0f, stage B %.0f, flush %.0f, unit records %.0f\n",
                    (double)t[4] / n_units, (double)t[5] / n_units, (double)t[6] / n_units, (double)t[7] / n_units, (double)t[8] / n_units,
                    (double)t[9] / n_units, (double)t[10] / n_units, (double)t[11] / n_units);
        else
            fprintf(stderr, "[gft scan debug] wave cycles per unit: first bytes %.0f, filter %.0f, list %.0f, stage A %.0f (scan5: trips %.0f + stage-B issue and short-term trips %.0f), stage B %.0f, flush %.0f, unit record %.0f\n",
                (double)t[4] / n_units, (double)t[5] / n_units, (double)t[6] / n_units, (double)(t[7] + t[10]) / n_units, (double)t[10] / n_units, (double)t[7] / n_units,
                (double)t[8] / n_units, (double)t[9] / n_units, (double)t[11] / n_units);
        double sum = 0;
        for (int ph = 4; ph < 12; ph++) sum += (double)t[ph];
        if (t[13]) fprintf(stderr, "[gft scan debug] %llu waves: mean %.0f cycles in all, the slowest %.0f (+%.1f %%)\n", (unsigned long long)t[13],
                           sum / (double)t[13], (double)t[12], 100.0 * ((double)t[12] * (double)t[13] / sum - 1.0));
    }
    return GFT_OK;
}

// What a completed batch teaches the next ones (batch_verdict.hpp)
static void learn_from_batch(gft_engine* e, const ScanLaunch& L, const BatchVerdict& v) {
    const ScanKernel k = e->plan.kernel;
    learn(e->learned, k, k == ScanKernel::scan5 ? e->plan.s5plan.fifo_cap : kScan2FifoCap, L.ordered, v.total, v.text_lo, v.text_hi);
    e->learned.unit_entries = v.n_units ? (uint32_t)std::min<uint64_t>((v.total + v.n_units - 1) / v.n_units, 0xFFFFFFFFu) : 0u;
}

// How a batch gets its unit table
enum class UnitRoute {
    host,       // computed on the host and uploaded: small batches from host memory
    single,     // ONE launch on the assumption that every document is one unit (k_units_single)
    deferred,   // count + prefix sum + fill + clamp into the table as the last batch left it; the true count is read afterwards
    counted,    // count + prefix sum, a read-back of the count, fill
};
constexpr const char* kUnitRouteName[] = {"host", "single", "deferred", "counted"};      // (in UnitRoute's order)
constexpr uint64_t kHostUnitDocs = 1024;   // batches up to this many documents get their unit table from the host

// What build_unit_table says of the table it made: the units the scan is launched over and the text range they cover.  The
// host route's arrays live here: the uploads read them until the stream has drained, on every way out of scan_pipeline.
struct UnitTable {
    gft_engine* e;
    uint64_t n_units = 0, text_lo = 0, text_hi = 0;
    std::vector<uint64_t> h_base;
    std::vector<Unit> h_units;
    bool drain = false;
    explicit UnitTable(gft_engine* e_) : e(e_) {}
    ~UnitTable() { if (drain && e->stream) (void)hipStreamSynchronize(e->stream); }
};

// 1. work units: sizes the buffers, puts on the stream what `route` needs, tells L what a deferred launch knew and t what
// the scan is launched over.  cap_units: the units the table holds as it is.
static int build_unit_table(gft_engine* e, UnitRoute route, const uint64_t* d_doc_off, const uint64_t* h_doc_off, uint64_t n_docs,
                            uint32_t unit_max, uint64_t cap_units, ScanLaunch& L, UnitTable& t) {
    hipStream_t st = e->stream;
    HIP_TRY(e->d_ctl.ensure(kCtlBytes), "control alloc");
    HIP_TRY(e->d_unit_cnt.ensure(n_docs * 4), "unit alloc");
    HIP_TRY(e->d_unit_base.ensure((n_docs + 1) * 8), "unit alloc");
    HIP_TRY(e->d_partial.ensure(scan_partials_needed(n_docs) * 8), "unit alloc");
    // (k_units_single also clears the control block -- its two flags are raised to the batch's EPOCH, a number no earlier batch
    // wrote there, so they need no clearing: one node less on the stream of every batch)
    if (route != UnitRoute::single) HIP_TRY(hipMemsetAsync(e->d_ctl.p, 0, kCtlBatchClear, st), "memset");
    // what is sized by the number of units, once the route knows it
    auto room = [&]() -> int {
        HIP_TRY(e->d_units.ensure(t.n_units * sizeof(Unit)), "unit alloc");
        HIP_TRY(e->d_unit_start.ensure(t.n_units * 8), "unit alloc");
        HIP_TRY(e->d_unit_count.ensure(t.n_units * 4), "unit alloc");
        HIP_TRY(e->d_unit_out.ensure((t.n_units + 1) * 8), "unit alloc");
        HIP_TRY(e->d_partial.ensure(scan_partials_needed(std::max(t.n_units, n_docs)) * 8), "unit alloc");
        return GFT_OK;
    };
    // units per document, their prefix sum, and the three numbers of the control block that come of them
    auto count = [&]() -> int {
        ProfScope ps(e, "aux");
        HIP_TRY(launch_unit_count(d_doc_off, n_docs, unit_max, e->d_unit_cnt.as<uint32_t>(), ctl_at<uint32_t>(e, kCtlBad), st), "unit_count");
        HIP_TRY(launch_exclusive_scan(e->d_unit_cnt.as<uint32_t>(), n_docs, e->d_unit_base.as<uint64_t>(),
                                      e->d_partial.as<uint64_t>(), st), "unit scan");
        HIP_TRY(launch_pack_ctl(e->d_unit_base.as<uint64_t>(), d_doc_off, n_docs, ctl_at<uint64_t>(e, kCtlUnits), st), "unit scan");
        return GFT_OK;
    };
    int rc;
    switch (route) {
    case UnitRoute::host: {
        // small batches from host memory (a single ProcessText / FindSubstrings call is the reference's own shape): the unit
        // table is a few entries, computed here and uploaded instead of five kernel launches and a synchronising read-back
        t.drain = true;
        t.h_base.assign(n_docs + 1, 0);
        for (uint64_t d = 0; d < n_docs; d++) {
            if (h_doc_off[d + 1] < h_doc_off[d]) return fail(e, GFT_E_INVALID, "doc_off is not ascending");
            const uint64_t n = h_doc_off[d + 1] - h_doc_off[d];
            if (n > 0xFFFFFFFFull) return fail(e, GFT_E_UNSUPPORTED, "a document is longer than 4 GiB - 1 bytes (positions are 32-bit)");
            const uint64_t k = n <= unit_max ? 1 : (n + unit_max - 1) / unit_max;
            t.h_base[d + 1] = t.h_base[d] + k;
            for (uint64_t i = 0; i < k; i++) t.h_units.push_back(unit_slice((uint32_t)d, n, k, i, unit_max));
        }
        t.n_units = t.h_base[n_docs]; t.text_lo = h_doc_off[0]; t.text_hi = h_doc_off[n_docs];
        HIP_TRY(hipMemcpyAsync(e->d_unit_base.p, t.h_base.data(), (n_docs + 1) * 8, hipMemcpyHostToDevice, st), "unit upload");
        if ((rc = room())) return rc;
        ProfScope ps(e, "aux");
        if (t.n_units) HIP_TRY(hipMemcpyAsync(e->d_units.p, t.h_units.data(), t.n_units * sizeof(Unit), hipMemcpyHostToDevice, st), "unit upload");
        return GFT_OK;
    }
    case UnitRoute::single: {
        // The batch before was one unit per document: this one gets its table on that assumption; deferred_interpret learns
        // whether it held
        {
            ProfScope ps(e, "aux");
            HIP_TRY(launch_units_single(d_doc_off, n_docs, unit_max, e->d_units.as<Unit>(), e->d_unit_base.as<uint64_t>(),
                                        ctl_at<uint32_t>(e, kCtlBad), e->ctl_epoch, st), "unit table");
        }
        t.n_units = n_docs; t.text_lo = 0; t.text_hi = ~0ull;
        L.deferred = L.single = true; L.epoch = e->ctl_epoch;
        L.unit_cap = L.n_docs = n_docs;
        if ((rc = room())) return rc;
        // (nothing to fill: the scope is empty.  It stays because every route has always opened two "aux" scopes a batch, and
        // that is the launch count gft_profile_read("aux") hands to the tools; no test reads it)
        ProfScope ps(e, "aux");
        return GFT_OK;
    }
    case UnitRoute::deferred: {
        // No read-back when the caller checks afterwards: the tables keep the size the last batch gave them (a document
        // is one unit unless it is longer than unit_max), units beyond the table are dropped and every index is clamped
        // into it -- deferred_interpret sees the true count and has the batch run again
        if ((rc = count())) return rc;
        L.deferred = true;
        t.n_units = cap_units; t.text_lo = 0; t.text_hi = ~0ull;       // (the text blob is readable 64 bytes past its end: gft.h)
        L.unit_cap = cap_units; L.n_docs = n_docs;
        if ((rc = room())) return rc;
        ProfScope ps(e, "aux");
        HIP_TRY(hipMemsetAsync(e->d_units.p, 0, t.n_units * sizeof(Unit), st), "memset");      // empty units behind the real ones
        HIP_TRY(launch_unit_fill(d_doc_off, n_docs, e->d_unit_base.as<uint64_t>(), e->d_units.as<Unit>(), unit_max, st, t.n_units), "unit_fill");
        HIP_TRY(launch_clamp_u64(e->d_unit_base.as<uint64_t>(), n_docs + 1, t.n_units, st), "unit clamp");
        return GFT_OK;
    }
    case UnitRoute::counted: {
        if ((rc = count())) return rc;
        uint64_t raw[kCtlWords] = {};
        HIP_TRY(hipMemcpyAsync(raw, e->d_ctl.p, sizeof raw, hipMemcpyDeviceToHost, st), "readback");
        HIP_TRY(hipStreamSynchronize(st), "sync");
        const CtlBlock c = decode_ctl(raw);
        t.n_units = c.n_units; t.text_lo = c.text_lo; t.text_hi = c.text_hi;
        count_streak(e->learned, t.n_units, n_docs);
        if (t.text_hi < t.text_lo) return fail(e, GFT_E_INVALID, "doc_off is not ascending");
        if (c.bad) return fail(e, GFT_E_INVALID, "doc_off is not ascending, or a document is longer than 4 GiB - 1 bytes (positions are 32-bit)");
        if ((rc = room())) return rc;
        ProfScope ps(e, "aux");
        HIP_TRY(launch_unit_fill(d_doc_off, n_docs, e->d_unit_base.as<uint64_t>(), e->d_units.as<Unit>(), unit_max, st), "unit_fill");
        return GFT_OK;
    }
    }
    return GFT_E_INTERNAL;
}

// The device pipeline shared by scan and process.  On success the canonical CSR sits in e->d_match_off / d_term / d_pos
// (need_csr) and `v` says what the scan established -- unless the launch was deferred: deferred_interpret then does.
// defer != nullptr: the launch may be deferred -- the caller reads the control block back itself after its last kernel
// (deferred_interpret), the unit table and the match pool are sized from the previous batch, and a batch that outgrew them is
// run again.  *defer says whether it was, and what the launch knew.
int scan_pipeline(gft_engine* e, const uint8_t* d_text, const uint64_t* d_doc_off, uint64_t n_docs, uint32_t flags,
                  bool need_csr, BatchVerdict& v, const uint64_t* h_doc_off, ScanLaunch* defer) {
    hipStream_t st = e->stream;
    v = BatchVerdict();                   // (an empty batch: nothing scanned, no range for refine_nonascii to judge)
    ScanLaunch L;
    if (defer) *defer = L;
    e->pool = PoolState();                // the pool is about to be overwritten
    e->solve_unit_entries = e->learned.unit_entries;     // (what the batches BEFORE this one taught: its solver plans with that)
    HIP_TRY(e->d_match_off.ensure((n_docs + 1) * 8), "match_off alloc");
    if (n_docs == 0) {
        HIP_TRY(hipMemsetAsync(e->d_match_off.p, 0, 8, st), "memset");
        HIP_TRY(hipStreamSynchronize(st), "sync");
        return GFT_OK;
    }
    const uint32_t warm = e->tables.tab.max_term_len ? e->tables.tab.max_term_len - 1 : 0;
    // gft_scan2: a unit's matches should fit the wave's LDS fifo (kScan2FifoCap), so the unit size follows the match
    // density the previous call saw (dense dictionaries -> smaller units); results do not depend on it
    const uint32_t unit_max = e->plan.kernel == ScanKernel::scan3 ? kScan3UnitMax : e->plan.kernel == ScanKernel::scan4 ? kScan4UnitMax
                              : on_scan2_tables(e->plan.kernel) ? e->learned.unit_max : kTextBuf - warm;

    // 1. work units.  A launch can be deferred when the caller asked for it, wants no CSR, and the unit table and the pool of
    // an earlier batch are there to run in; after two batches of one unit per document, k_units_single makes the table
    const uint64_t cap_units = std::min(std::min(e->d_units.cap / sizeof(Unit), e->d_unit_start.cap / 8), e->d_unit_count.cap / 4);
    const bool can_defer = defer && !need_csr && cap_units >= n_docs && e->pool_cap > 0;
    UnitRoute route = h_doc_off != nullptr && n_docs <= kHostUnitDocs ? UnitRoute::host
                      : can_defer && e->learned.single_streak >= 2    ? UnitRoute::single
                      : can_defer                                     ? UnitRoute::deferred
                                                                      : UnitRoute::counted;
    if (route == UnitRoute::single && ++e->ctl_epoch < 2) { e->ctl_epoch = 1; route = UnitRoute::deferred; }      // (wrapped: this batch the general way)
    e->last_unit_route = kUnitRouteName[(int)route];
    UnitTable table(e);
    int rc = build_unit_table(e, route, d_doc_off, h_doc_off, n_docs, unit_max, cap_units, L, table);
    if (rc) return rc;
    const uint64_t n_units = table.n_units, text_lo = table.text_lo, text_hi = table.text_hi;
    if (!L.deferred) { v.text_lo = text_lo; v.text_hi = text_hi; }

    // 2. automaton walk into the slab pool; grow the pool and re-run if it overflowed (never truncate)
    const ScanKernel k = e->plan.kernel;
    if (L.deferred) L.pool_cap = e->pool_cap;
    rc = L.deferred ? GFT_OK : ensure_pool(e, std::max<uint64_t>(1u << 20, (text_hi - text_lo) / 16));
    if (!rc && !L.deferred && counts_slabs(k)) {
        // (every wave of the grid owns a slab from the start: the pool holds those twice over, or a small batch on a fresh
        // engine would overflow it before it had written a match)
        // (scan4: a slab holds at least one chunk's regions -- up to eight units of unit_max bytes at 1.6 x the density seen)
        const uint64_t min_slab = k == ScanKernel::scan4 ? kScan4ChunkUnits * ((uint64_t)(unit_max * e->learned.scan4_density * 1.6) + 49) : slab_floor(k);
        rc = ensure_pool(e, 2 * grid_waves(e, n_units) * min_slab);
    }
    if (rc) return rc;
    const ScanBatch batch{d_text, d_doc_off, n_docs, n_units, text_hi, flags, unit_max, need_csr};
    uint64_t total = 0;
    for (int attempt = 0; attempt < 3; attempt++) {
        if (attempt) HIP_TRY(hipMemsetAsync(ctl_at<uint8_t>(e, kCtlCursor), 0, kCtlRetryClear, st), "memset");
        if ((rc = enqueue_scan(e, batch, L))) return rc;
        if (L.deferred) { *defer = L; return GFT_OK; }         // (the caller reads the cursor back after the solver)
        uint64_t raw[kCtlWords] = {};                          // (the words behind the scan alone: cursor, match count, non-ASCII bits)
        HIP_TRY(hipMemcpyAsync(raw + kCtlCursor / 8, ctl_at<uint8_t>(e, kCtlCursor), kCtlScanRead, hipMemcpyDeviceToHost, st), "readback");
        HIP_TRY(hipStreamSynchronize(st), "scan kernel");
        const CtlBlock c = decode_ctl(raw);
        const uint64_t cursor = c.cursor + L.static_slabs;
        total = counts_slabs(k) ? c.total : c.cursor;          // (the DFA kernel keeps no count of its own: its cursor is that)
        v.nonascii_bits = c.nonascii_bits; v.nonascii = c.nonascii_bits != 0;
        if (on_scan2_tables(k) && (e->opt_scan_dbg & 2)) {
            uint64_t c4[4] = {0, 0, 0, 0};
            HIP_TRY(hipMemcpy(c4, e->d_dbg.p, 32, hipMemcpyDeviceToHost), "debug readback");
            fprintf(stderr, "[gft scan debug] units=%llu flagged=%llu sum_of_per_unit_max_lane=%llu to_bucket_table=%llu matches=%llu\n",
                    (unsigned long long)n_units, (unsigned long long)c4[0], (unsigned long long)c4[1],
                    (unsigned long long)c4[2], (unsigned long long)total);
        }
        v.n_units = n_units; v.total = total;
        if (cursor <= e->pool_cap) { learn_from_batch(e, L, v); break; }
        if (attempt == 2) return fail(e, GFT_E_HIP, "match pool overflow persisted");
        rc = ensure_pool(e, cursor + cursor / 16);
        if (rc) return rc;
    }

    e->pool.n_units = n_units; e->pool.total = total;
    if (!need_csr) return GFT_OK;   // the solver reads the slabs in place (doc -> units -> pool)
    return csr_from_pool(e, n_docs);
}

// The verdict on a deferred launch (scan_pipeline) from the read-back of the control block that its caller made after the
// batch's last kernel: judge_deferred says it, this applies it.  *again = the unit table or the match pool was too small
// (the pool has been grown): the caller runs the batch once more, this time with the sizes known.
int deferred_interpret(gft_engine* e, const uint64_t* raw, const ScanLaunch& L, BatchVerdict& v, bool* again) {
    const CtlBlock c = decode_ctl(raw);
    const Judgement j = judge_deferred(c, L);
    v = j.verdict;
    *again = j.kind == Judgement::again_general || j.kind == Judgement::again_grow;
    if (single_miss(c, L)) { e->learned.single_streak = kSingleMissStreak; return GFT_OK; }
    count_streak(e->learned, v.n_units, L.n_docs);
    e->pool.n_units = v.n_units; e->pool.total = v.total;
    if (j.kind == Judgement::invalid) return fail(e, GFT_E_INVALID, j.err);
    if (j.kind == Judgement::again_grow) return ensure_pool(e, j.pool_need);     // (a no-op when it has grown past the need since)
    if (j.kind == Judgement::accept) learn_from_batch(e, L, v);
    return GFT_OK;
}

// A folded scan that met bytes >= 0x80: is ASCII folding still the whole of strings.ToLower for this text (k_fold_safe)?
// One more pass over the text and one more read-back, for such batches only.
int refine_nonascii(gft_engine* e, const uint8_t* d_text, const uint64_t* d_doc_off, uint64_t n_docs, uint32_t flags, BatchVerdict& v) {
    if (!(flags & GFT_FOLD_ASCII)) { v.nonascii = false; return GFT_OK; }
    if (!v.nonascii) return GFT_OK;
    // (gft_scan3 / gft_scan5 judge the pieces that hold high bytes themselves -- gft_foldsafe_dev.hpp -- and say "unsafe"
    // or nothing; the other kernels only say that they saw some)
    if (!(v.nonascii_bits & 1u)) { v.nonascii = (v.nonascii_bits & 2u) != 0; return GFT_OK; }
    uint32_t flag = 0;
    uint32_t* d_flag = ctl_at<uint32_t>(e, kCtlNonascii);
    {
        ProfScope ps(e, "aux");
        // (the word starts at zero: a younger batch in flight may have left its own bits there since this batch's scan)
        HIP_TRY(hipMemsetAsync(d_flag, 0, 4, e->stream), "memset");
        HIP_TRY(launch_fold_safe(d_text, v.text_lo, v.text_hi, d_doc_off, n_docs, d_flag, e->stream), "fold check");
    }
    HIP_TRY(hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, e->stream), "readback");
    HIP_TRY(hipStreamSynchronize(e->stream), "fold check");
    v.nonascii = (flag & 2u) != 0;
    return GFT_OK;
}

// GFT_SCAN_UNIQUE: the canonical CSR in d_match_off / d_term -> every term once per document, first occurrences in order.
// The result replaces d_match_off / d_term (positions: zeros in d_pos); *n_matches = new total.
int unique_pipeline(gft_engine* e, uint64_t n_docs, uint64_t* n_matches) {
    if (!n_docs) return GFT_OK;
    hipStream_t st = e->stream;
    const uint32_t n_terms = std::max<uint32_t>((uint32_t)e->tables.tab.terms.size(), 1);
    // as many workgroups as 256 MB of first-occurrence rows allow, at most 4 per CU
    const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(n_docs, (uint64_t)e->n_cus * 4), (256ull << 20) / ((uint64_t)n_terms * 4)));
    HIP_TRY(e->d_uq.first.ensure((size_t)grid * n_terms * 4), "unique alloc");
    HIP_TRY(e->d_uq.cnt.ensure(n_docs * 4), "unique alloc");
    HIP_TRY(e->d_uq.off.ensure((n_docs + 1) * 8), "unique alloc");
    HIP_TRY(e->d_partial.ensure(scan_partials_needed(n_docs) * 8), "unique alloc");
    HIP_TRY(hipMemsetAsync(e->d_uq.first.p, 0xFF, (size_t)grid * n_terms * 4, st), "memset");
    ProfScope ps(e, "aux");
    HIP_TRY(launch_unique_terms(false, e->d_match_off.as<uint64_t>(), e->d_term.as<uint32_t>(), n_docs, n_terms, e->d_uq.first.as<uint32_t>(), grid,
                                e->d_uq.cnt.as<uint32_t>(), nullptr, nullptr, st), "unique count");
    HIP_TRY(launch_exclusive_scan(e->d_uq.cnt.as<uint32_t>(), n_docs, e->d_uq.off.as<uint64_t>(), e->d_partial.as<uint64_t>(), st), "unique scan");
    uint64_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, e->d_uq.off.as<uint64_t>() + n_docs, 8, hipMemcpyDeviceToHost, st), "readback");
    HIP_TRY(hipStreamSynchronize(st), "unique scan");
    HIP_TRY(e->d_uq.term.ensure(std::max<uint64_t>(total, 1) * 4), "unique alloc");
    HIP_TRY(launch_unique_terms(true, e->d_match_off.as<uint64_t>(), e->d_term.as<uint32_t>(), n_docs, n_terms, e->d_uq.first.as<uint32_t>(), grid,
                                nullptr, e->d_uq.off.as<uint64_t>(), e->d_uq.term.as<uint32_t>(), st), "unique write");
    // the caller-visible buffers: offsets and terms are swapped in, positions are all zero (substringEngine.go:83)
    std::swap(e->d_match_off, e->d_uq.off);
    std::swap(e->d_term, e->d_uq.term);
    HIP_TRY(e->d_pos.ensure(std::max<uint64_t>(total, 1) * 4), "unique alloc");
    HIP_TRY(hipMemsetAsync(e->d_pos.p, 0, std::max<uint64_t>(total, 1) * 4, st), "memset");
    *n_matches = total;
    return GFT_OK;
}

// GFT_POS_RUNES: the positions of the canonical CSR in d_pos become offsets over []rune(text), what AnknownEngine reports
// (finder/substringEngine.go:44-53: MultiPatternSearch([]rune(text), ...), Position = m.Pos)
int rune_pipeline(gft_engine* e, const uint8_t* d_text, const uint64_t* d_doc_off, uint64_t n_docs, uint64_t n_matches) {
    if (!n_docs || !n_matches) return GFT_OK;
    hipStream_t st = e->stream;
    HIP_TRY(e->d_rn.cnt.ensure(n_docs * 4), "rune alloc");
    HIP_TRY(e->d_rn.base.ensure((n_docs + 1) * 8), "rune alloc");
    HIP_TRY(e->d_partial.ensure(scan_partials_needed(n_docs) * 8), "rune alloc");
    ProfScope ps(e, "aux");
    HIP_TRY(launch_rune_doc_blocks(d_doc_off, n_docs, e->d_rn.cnt.as<uint32_t>(), st), "rune blocks");
    HIP_TRY(launch_exclusive_scan(e->d_rn.cnt.as<uint32_t>(), n_docs, e->d_rn.base.as<uint64_t>(), e->d_partial.as<uint64_t>(), st), "rune scan");
    uint64_t n_blocks = 0;
    HIP_TRY(hipMemcpyAsync(&n_blocks, e->d_rn.base.as<uint64_t>() + n_docs, 8, hipMemcpyDeviceToHost, st), "readback");
    HIP_TRY(hipStreamSynchronize(st), "rune scan");
    HIP_TRY(e->d_rn.starts.ensure(std::max<uint64_t>(n_blocks, 1) * 4), "rune alloc");
    HIP_TRY(e->d_rn.prefix.ensure((n_blocks + 1) * 8), "rune alloc");
    HIP_TRY(e->d_partial.ensure(scan_partials_needed(std::max(n_blocks, n_docs)) * 8), "rune alloc");
    HIP_TRY(launch_rune_block_starts(d_text, d_doc_off, e->d_rn.base.as<uint64_t>(), n_docs, n_blocks, e->d_rn.starts.as<uint32_t>(), st), "rune starts");
    HIP_TRY(launch_exclusive_scan(e->d_rn.starts.as<uint32_t>(), n_blocks, e->d_rn.prefix.as<uint64_t>(), e->d_partial.as<uint64_t>(), st), "rune scan");
    HIP_TRY(launch_pos_to_rune(d_text, d_doc_off, e->d_rn.base.as<uint64_t>(), e->d_rn.prefix.as<uint64_t>(), e->d_match_off.as<uint64_t>(), n_docs,
                               n_matches, e->d_pos.as<uint32_t>(), st), "rune offsets");
    return GFT_OK;
}

int solve_pipeline(gft_engine* e, uint64_t n_docs, const gft_extra_matches* d_extra, uint32_t* d_bitmap) {
    if (!n_docs || !e->n_exprs) return GFT_OK;
    SolveParams S;
    S.doc_unit_base = e->d_unit_base.as<uint64_t>();
    S.unit_start = e->d_unit_start.as<uint64_t>(); S.unit_count = e->d_unit_count.as<uint32_t>();
    S.units = e->d_units.as<Unit>();
    S.has_rare = e->progs.n_rare_words > 0 ? 1u : 0u;
    S.pos_back = (e->build_flags & GFT_POS_END) ? 0u : (e->tables.tab.max_term_len ? e->tables.tab.max_term_len - 1 : 0u);
    S.term = e->d_pool_term.as<uint32_t>(); S.pos = e->d_pool_pos.as<uint32_t>();
    S.x_off = d_extra ? d_extra->off : nullptr;
    S.x_slot = d_extra ? d_extra->slot : nullptr;
    S.x_pos = d_extra ? d_extra->pos : nullptr;
    S.n_docs = n_docs;
    const gft_engine::ProgramBufs& d = e->d_progs;
    S.fprog = d.fprog.as<uint32_t>(); S.fprog_off = d.fprog_off.as<uint64_t>();
    S.gprog = d.prog.as<uint32_t>(); S.groups = d.groups.as<uint32_t>();
    S.order = d.order.as<uint32_t>(); S.blk_class = d.blk_class.as<uint32_t>(); S.wave_blk = d.wave_blk.as<uint32_t>();
    S.fprog_t = d.fprog_t.as<uint32_t>(); S.fblk_off = d.fblk_off.as<uint32_t>();
    S.n_exprs = e->n_exprs;
    S.n_slots = (uint32_t)e->tables.tab.terms.size() + e->n_extra + 1;
    S.bitmap = d_bitmap;
    S.p_scratch = nullptr;
    S.dbg = e->opt_solve.dbg;
    S.dbg_out = nullptr;
    if (S.dbg & 8) {
        HIP_TRY(e->d_solve_dbg.ensure(128 * 8), "debug alloc");
        HIP_TRY(hipMemsetAsync(e->d_solve_dbg.p, 0, 128 * 8, e->stream), "memset");
        S.dbg_out = e->d_solve_dbg.as<unsigned long long>();
    }
    S.fprog_words = e->progs.fprog_words;
    SolveShape shape;
    shape.n_slots = S.n_slots; shape.n_exprs = S.n_exprs; shape.fprog_words = S.fprog_words;
    shape.has_rare = S.has_rare; shape.wide_pairs = e->progs.wide_pairs;
    shape.unit_entries = e->solve_unit_entries;        // (the batch before: a deferred scan's own count is read back behind its solver)
    const SolvePlan plan = plan_solve(shape, e->lds_max, e->n_cus, n_docs, e->opt_solve);
    S.tile_words = plan.tile_words;
    e->last_pf_terms = plan.pf_terms;
    if (!plan.p_in_lds) {
        HIP_TRY(e->d_pscratch.ensure((size_t)plan.grid * S.n_slots * 8), "presence scratch alloc");
        S.p_scratch = e->d_pscratch.as<uint64_t>();
    }
    S.wide_slot = nullptr; S.wide_theta = nullptr; S.wide_cap = plan.wide_cap; S.wide_list = nullptr; S.n_wide = 0;
    if (plan.wide_cap) {
        // (a region per wave of the grid; 12 bytes per pair: 8 192 pairs x 4 096 waves = 400 MB at the very most)
        const uint64_t n_waves = (uint64_t)plan.grid * (kSolveBlockThreads / 64);
        HIP_TRY(e->d_wide_slot.ensure(n_waves * S.wide_cap * 4), "INORD scratch alloc");
        HIP_TRY(e->d_wide_theta.ensure(n_waves * S.wide_cap * 8), "INORD scratch alloc");
        S.wide_slot = e->d_wide_slot.as<uint32_t>();
        S.wide_theta = e->d_wide_theta.as<long long>();
        S.wide_list = d.wide_list.as<uint32_t>(); S.n_wide = e->progs.n_wide;
    }
    ProfScope ps(e, "solve");
    HIP_TRY(launch_solve(S, plan, e->stream), "solve kernel launch");
    if (S.dbg & 8) {
        // phase clocks: cycles per group and wave (0 build, 1 barrier, 2 evaluation, 3 barrier, 4 transpose + wipe, 5 barrier,
        // 6 bitmap rows, 7 loop head), averaged over the workgroups
        unsigned long long t[128];
        HIP_TRY(hipMemcpyAsync(t, e->d_solve_dbg.p, sizeof t, hipMemcpyDeviceToHost, e->stream), "debug read-back");
        HIP_TRY(hipStreamSynchronize(e->stream), "debug read-back");
        const uint64_t n_groups = (n_docs + plan.group_docs - 1) / plan.group_docs;
        fprintf(stderr, "[gft solve debug] cycles per group: wave | build bar eval bar transpose bar rows head\n");
        for (int w = 0; w < 16; w++) {
            fprintf(stderr, "[gft solve debug] %2d |", w);
            for (int ph = 0; ph < 8; ph++) fprintf(stderr, " %7.0f", (double)t[w * 8 + ph] / (double)n_groups);
            fprintf(stderr, "\n");
        }
    }
    return GFT_OK;
}

// ---- what the host solves (host_solve.hpp) ---------------------------------------------------------------------------
// extra: the caller's matches as HOST arrays (nullable).  A slot's list is what addMatchesToSolverMap builds
// (finder/finder.go:181-196): the scan's positions of the term, then the caller's in the order given.  It can only be out
// of order when the caller's matches name a dictionary term (a regex with the text of a keyword), or are themselves not
// ascending (a foreign engine's keyword hits followed by the regex engine's for the same literal).
void plan_host(const gft_engine* e, const gft_extra_matches* extra, uint64_t n_docs, HostPlan& plan) {
    plan.all_docs = !e->progs.host_only.empty();
    plan.irregular.clear();
    if (!extra || !extra->off || e->progs.inord_exprs.empty() || !n_docs) return;
    const uint32_t n_terms = (uint32_t)e->tables.tab.terms.size();
    std::vector<std::pair<uint32_t, uint32_t>> seen;          // (slot, last position) of this document: a handful
    for (uint64_t d = 0; d < n_docs; d++) {
        seen.clear();
        bool irr = false;
        for (uint64_t i = extra->off[d]; i < extra->off[d + 1] && !irr; i++) {
            const uint32_t sl = extra->slot[i];
            if (sl >= e->progs.inord_slot.size() || !e->progs.inord_slot[sl]) continue;      // (range errors are upload_extra's to report)
            if (sl < n_terms) { irr = true; break; }
            size_t k = 0;
            while (k < seen.size() && seen[k].first != sl) k++;
            if (k == seen.size()) seen.emplace_back(sl, extra->pos[i]);
            else { irr = extra->pos[i] < seen[k].second; seen[k].second = extra->pos[i]; }
        }
        if (irr) plan.irregular.push_back(d);
    }
}

// Solve the planned (expression, document) pairs on the host from the scan's matches and the caller's, and put their bits
// into the bitmap: h_bitmap (host rows, already downloaded) or d_bitmap (device rows, patched by a small kernel).
int host_eval(gft_engine* e, const gft_extra_matches* extra, uint64_t n_docs, const HostPlan& plan, uint32_t* h_bitmap,
              uint32_t* d_bitmap) {
    if (plan.empty() || !n_docs || !e->n_exprs) return GFT_OK;
    hipStream_t st = e->stream;
    if (!e->pool.csr_valid) { int rc = csr_from_pool(e, n_docs); if (rc) return rc; }
    std::vector<uint64_t> mo(n_docs + 1);
    HIP_TRY(hipMemcpyAsync(mo.data(), e->d_match_off.p, (n_docs + 1) * 8, hipMemcpyDeviceToHost, st), "download");
    HIP_TRY(hipStreamSynchronize(st), "host solve");
    // the matches of the documents in question: all of them, or the irregular documents' ranges
    std::vector<uint64_t> docs;
    if (plan.all_docs) { docs.resize(n_docs); for (uint64_t d = 0; d < n_docs; d++) docs[d] = d; }
    else docs = plan.irregular;
    std::vector<uint32_t> ti, po;
    std::vector<uint64_t> at(docs.size() + 1, 0);           // document k's matches: [at[k], at[k + 1]) of ti / po
    for (size_t k = 0; k < docs.size(); k++) at[k + 1] = at[k] + (mo[docs[k] + 1] - mo[docs[k]]);
    ti.resize(at.back() + 1); po.resize(at.back() + 1);
    if (plan.all_docs) {
        if (at.back()) {
            HIP_TRY(hipMemcpyAsync(ti.data(), e->d_term.p, at.back() * 4, hipMemcpyDeviceToHost, st), "download");
            HIP_TRY(hipMemcpyAsync(po.data(), e->d_pos.p, at.back() * 4, hipMemcpyDeviceToHost, st), "download");
        }
    } else {
        for (size_t k = 0; k < docs.size(); k++) {
            const uint64_t n = at[k + 1] - at[k];
            if (!n) continue;
            HIP_TRY(hipMemcpyAsync(ti.data() + at[k], e->d_term.as<uint32_t>() + mo[docs[k]], n * 4, hipMemcpyDeviceToHost, st), "download");
            HIP_TRY(hipMemcpyAsync(po.data() + at[k], e->d_pos.as<uint32_t>() + mo[docs[k]], n * 4, hipMemcpyDeviceToHost, st), "download");
        }
    }
    HIP_TRY(hipStreamSynchronize(st), "host solve");
    const uint64_t words = (e->n_exprs + 31) / 32;
    std::vector<uint64_t> pw;                                // patches for a device bitmap: word index, bits to clear, bits to set
    std::vector<uint32_t> pclr, pset;
    SlotLists lists;
    size_t ir = 0;                                           // next irregular document
    for (size_t k = 0; k < docs.size(); k++) {
        const uint64_t d = docs[k];
        while (ir < plan.irregular.size() && plan.irregular[ir] < d) ir++;
        const bool irregular = ir < plan.irregular.size() && plan.irregular[ir] == d;
        // sortedMatchesByKeyword of this document (finder/finder.go:181-196): the engine's matches first (emission order:
        // ascending per term), the caller's behind them in the order given
        lists.clear();
        for (uint64_t i = at[k]; i < at[k + 1]; i++) lists[ti[i]].push_back((int64_t)po[i]);
        if (extra && extra->off)
            for (uint64_t i = extra->off[d]; i < extra->off[d + 1]; i++) lists[extra->slot[i]].push_back((int64_t)extra->pos[i]);
        auto solve_one = [&](uint32_t x) {
            const bool hit = host_solve(e->progs.prog.data() + e->progs.prog_off[x], e->progs.prog_off[x + 1] - e->progs.prog_off[x], lists);
            const uint64_t w = d * words + (x >> 5);
            const uint32_t bit = 1u << (x & 31);
            if (h_bitmap) h_bitmap[w] = hit ? h_bitmap[w] | bit : h_bitmap[w] & ~bit;
            else { pw.push_back(w); pclr.push_back(hit ? 0u : bit); pset.push_back(hit ? bit : 0u); }
        };
        for (uint32_t x : e->progs.host_only) solve_one(x);
        if (irregular) for (uint32_t x : e->progs.inord_exprs) solve_one(x);
    }
    if (!h_bitmap && !pw.empty()) {
        if (!d_bitmap) return fail(e, GFT_E_INVALID, "null bitmap");
        const size_t n = pw.size();
        HIP_TRY(e->d_patch.ensure(n * 16), "patch alloc");
        uint8_t* base = e->d_patch.as<uint8_t>();
        HIP_TRY(hipMemcpyAsync(base, pw.data(), n * 8, hipMemcpyHostToDevice, st), "patch upload");
        HIP_TRY(hipMemcpyAsync(base + n * 8, pclr.data(), n * 4, hipMemcpyHostToDevice, st), "patch upload");
        HIP_TRY(hipMemcpyAsync(base + n * 12, pset.data(), n * 4, hipMemcpyHostToDevice, st), "patch upload");
        HIP_TRY(launch_patch_words(d_bitmap, reinterpret_cast<const uint64_t*>(base), reinterpret_cast<const uint32_t*>(base + n * 8),
                                   reinterpret_cast<const uint32_t*>(base + n * 12), n, st), "patch");
        HIP_TRY(hipStreamSynchronize(st), "patch");
    }
    return GFT_OK;
}

}  // namespace gft::api
