// gft_api.cpp -- the C ABI of include/gft.h: engine handle, table upload, workspace management and the
// kernel pipelines behind gft_scan* / gft_process*.  Host orchestration only; all per-byte and per-match work
// happens in gft_kernels.hip.  There is no CPU fallback: every compute entry point needs a HIP device.
#include "../../include/gft.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_set>
#include <vector>

#include <cstdlib>

#include "batch_verdict.hpp"
#include "compact_host.hpp"
#include "copy_pool.hpp"
#include "gft_guard.hpp"
#include "gft_kernels.hpp"
#include "gft_rules.hpp"
#include "gft_tolower.hpp"
#include "host_solve.hpp"
#include "program_set.hpp"
#include "rule_set.hpp"
#include "table_set.hpp"

using namespace gft;

namespace {

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) { hipError_t e = hipFree(p); p = nullptr; cap = 0; if (e != hipSuccess) return e; }
        size_t want = bytes + bytes / 8 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

struct ProfCat {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
};

// What the unit table, the match pool and the result buffers hold now
struct PoolState {
    uint64_t n_units = 0, total = 0;       // of the last completed scan (csr_from_pool)
    uint64_t valid_docs = ~0ull;           // documents of the last gft_process scan still in the pool (~0: none)
    bool csr_valid = false;                // d_match_off / d_term / d_pos hold that scan's canonical CSR
};

}  // namespace

#ifndef GFT_EXTRA_KERNELS
// The earlier suffix-window kernels (gft_scan2.hip, gft_scan4.hip) are cross-checks and study objects: a product build
// does not carry them (python -m gofindthem_amd.build with GFT_EXTRA_KERNELS=1 does).  Without them nothing "fits".
namespace gft {
bool scan2_plan(uint32_t, uint32_t, uint32_t, uint32_t, size_t, uint32_t*, uint32_t*) { return false; }
hipError_t launch_scan2(const Scan2Params&, uint32_t, unsigned, hipStream_t) { return hipErrorNotSupported; }
bool scan4_plan(uint32_t, uint32_t, uint32_t, uint32_t, size_t, bool, uint32_t*, uint32_t*) { return false; }
hipError_t launch_scan4(const Scan2Params&, uint32_t, unsigned, hipStream_t) { return hipErrorNotSupported; }
}  // namespace gft
static constexpr bool kExtraKernels = false;
#else
static constexpr bool kExtraKernels = true;
#endif

struct gft_engine {
    int device = 0;
    hipStream_t stream = nullptr;
    // host -> device staging of large caller buffers: two pinned bounce buffers, filled by a few copy threads while the
    // previous one is on the wire (a hipMemcpy from pageable memory stages through one thread)
    void* pin[2] = {nullptr, nullptr};
    uint64_t* pin_rb = nullptr;            // pinned landing place of the per-batch read-back of the control block
    hipEvent_t pin_ev[2] = {nullptr, nullptr};
    std::unique_ptr<gft::CopyPool> copy_pool;   // the threads that fill / empty the bounce buffers (created with the first large copy)
    bool own_stream = false;
    unsigned n_cus = 256;                  // CUs the persistent kernels fill: the device's minus cu_margin
    unsigned n_cus_hw = 256, cu_margin = 0;
    size_t lds_max = 65536;
    mutable std::string err;

    // the dictionary (table_set.hpp): the compiled tables, the scan kernel chosen for them on this device with its LDS plan
    // and what scan5 derives from them; d_tabs: the copies on the device of what the DFA kernel, the gather (term_len) and
    // the chosen kernel read
    gft::TableSet tables;
    gft::ScanPlan plan;
    Scan5Tables s5;
    bool built = false;
    uint32_t build_flags = 0;
    struct TableBufs {
        struct { DevBuf byte_class, delta, out_term, out_link, term_len; } dfa;
        struct { DevBuf filter, slots, more, cls, cls_fold, term_blob, term_off, short3, shorts_packed, short3_big, fpt; } s2;
        struct { DevBuf filter, short3, srec, short3_big, srec_big, bloom, slots, more, cls, cls_fold, term_blob, term_off; } s3;
        struct { DevBuf grp, grp_fold, filter, bloom; } s5;
    } d_tabs;
    DevBuf d_ctl, d_dbg;                                // the control block (batch_verdict.hpp); GFT_SCAN_DEBUG counters
    // batch_verdict.hpp: what the batches taught the next ones; the verdict of the batch whose entry point returned last
    // (gft_last_nonascii) -- the public entry points assign it as their last act, nothing else does
    gft::Learned learned;
    gft::BatchVerdict reported;
    PoolState pool;
    // Environment switches (cross-checks and timing studies) are read when the handle is created and again
    // by gft_build / gft_import_tables / gft_set_programs -- never on the per-batch path
    uint32_t opt_scan_dbg = 0;                          // GFT_SCAN_DEBUG (timing studies)
    uint32_t opt_scan_prio = 1;                         // graded wave priorities in the scan kernels (GFT_SCAN_PRIO=0: off)
    uint32_t opt_scan_ordered = 0;                      // GFT_SCAN_ORDERED=1: scan2's per-lane staging path for every unit
    uint32_t opt_scan4_round = 0;                       // GFT_SCAN4_ROUND: bytes per lane and round of the streaming kernel (0: 64)
    uint32_t opt_scan4_chunk = 0;                       // GFT_SCAN4_CHUNK: units per chunk of the streaming kernel (0: by batch size)
    gft::SolveOptions opt_solve;                        // GFT_SOLVE_GROUP_DOCS, GFT_SOLVE_PROG_LDS, GFT_SOLVE_DEBUG (solve_plan.hpp)
    // one caller at a time per handle: every entry point that touches the device state takes this
    mutable std::recursive_mutex mu;
    // multi-device handle (gft_engine_create_multi): this engine serves devices[0], `peers` the others.  Tables and
    // programs are replicated, a batch is cut into contiguous document ranges of near-equal text bytes, every device
    // has its own host thread and stream for the duration of a call
    std::vector<gft_engine*> peers;
    std::vector<uint64_t> shard_cut;                     // document cuts of the last multi-device gft_process
    bool in_multi = false;                               // set while a multi-device call runs this engine's own share
    std::vector<void*> comms;                            // RCCL communicators (ncclCommInitAll), one per device; empty: none
    bool rccl_self = false;                              // GFT_RCCL_SELF=1 over one device named several times: ONE communicator of one rank
    void* rccl_lib = nullptr;

    // programs
    bool have_programs = false;
    uint32_t n_exprs = 0, n_extra = 0;
    gft::ProgramSet progs;                 // the installed set (program_set.hpp) ...
    struct ProgramBufs {                   // ... and the copies of its arrays that the solver kernel reads
        DevBuf prog, prog_off;             // public postfix words (INORD group subtrees are read from these)
        DevBuf fprog, fprog_off, groups;   // fused internal form + INORD group table
        DevBuf order, blk_class, wave_blk; // evaluation order of the programs
        DevBuf fprog_t, fblk_off;          // fused programs per sorted block of 64, transposed (read when they do not fit LDS)
        DevBuf wide_list;
    } d_progs;
    DevBuf d_patch;                        // bit patches of host-solved results for a device-resident bitmap
    DevBuf d_wide_slot, d_wide_theta;      // pairs of wide INORD groups, a region per wave of the solver's grid
    DevBuf d_solve_dbg;                    // GFT_SOLVE_DEBUG & 8: phase clocks
    uint32_t ctl_epoch = 1;                // k_units_single batches are numbered from 2 (their control-block flags)
    // gft_process_device_begin / _end: up to two batches enqueued, their read-backs landing in pinned slots of their own
    struct Pending {
        bool done = false;                 // completed inside begin (a batch that could not be deferred): rc is its status
        int rc = 0;
        const uint8_t* d_text = nullptr; const uint64_t* d_doc_off = nullptr; uint64_t n_docs = 0; uint32_t flags = 0;
        uint32_t* d_bitmap = nullptr;
        ScanLaunch launch;
        uint64_t* rb = nullptr; hipEvent_t ev = nullptr;
        gft::BatchVerdict verdict;         // the batch's own, complete when `done` or judged: what its _end reports
    };
    Pending pend[2];
    unsigned pend_head = 0, pend_count = 0;
    DevBuf d_pscratch;                    // HBM presence matrices when n_slots * 8 B does not fit LDS

    // workspace
    DevBuf d_unit_cnt, d_unit_base, d_units, d_partial, d_pool_term, d_pool_pos, d_unit_start,
        d_unit_count, d_unit_out, d_term, d_pos, d_match_off;
    uint64_t pool_cap = 0;
    // staging for the host-buffer entry points
    DevBuf d_text, d_doc_off, d_bitmap, d_xoff, d_xslot, d_xpos;
    DevBuf d_uq_first, d_uq_cnt, d_uq_off, d_uq_term;   // GFT_SCAN_UNIQUE: per-workgroup first-occurrence rows, unique CSR
    DevBuf d_rn_cnt, d_rn_base, d_rn_starts, d_rn_prefix;   // GFT_POS_RUNES: blocks per document, their rune starts, prefix sums
    std::vector<uint64_t> h_match_off;
    std::vector<uint32_t> h_term, h_pos;
    // sparse results (gft_compact.hip): a label per expression (gft_set_expr_labels), the compaction's scratch -- counts and
    // scan partials of its own, so that it may run beside batches in flight --, and the CSR of gft_process_sparse
    bool have_labels = false;
    std::vector<uint32_t> h_labels;
    DevBuf d_labels, d_cp_cnt, d_cp_partial, d_cp_row_off, d_cp_idx, d_cp_label;
    std::vector<uint64_t> h_row_off;
    std::vector<uint32_t> h_expr_idx, h_label, h_sparse_bm;
    // strings.ToLower on the device (gft_tolower.hip): the mapping table (uploaded with the first call), a unit table, counts
    // and scan partials of its own, and the lowered batch the finder scans again (gft_lower_owned)
    bool lower_table_up = false;
    DevBuf d_lw_page, d_lw_delta, d_lw_doc_units, d_lw_unit_base, d_lw_units, d_lw_partial, d_lw_unit_cnt, d_lw_unit_out, d_lw_ctl,
        d_lw_text, d_lw_off;

    // rule evaluation for records (gft_rules.hip): the installed set's shape and its arrays on the device, the leaf bitmap and
    // the tag rows of a batch, the flag words, staging for the host-pointer entry points
    struct RuleBufs {
        uint64_t serial = 0;               // 0: none installed
        uint32_t n_fields = 0, n_tags = 0, n_exprs = 0, n_rules = 0, n_units = 0, max_depth = 0, field_words = 0;
        DevBuf expr_tag, masks, units, prog, prog_off, leaf_bitmap, tag_rows, flags, stage[6];
    } d_rules;

    // profiling
    int profiling = 0;                     // gft_profile_enable: 0 off, 1 every category, 2 the scan kernel only
    std::vector<hipEvent_t> prof_pool;     // events given back by gft_profile_reset
    std::map<std::string, ProfCat> prof;
};

namespace {

long env_num(const char* name, long dflt) { const char* v = getenv(name); return v ? atol(v) : dflt; }

void refresh_options(gft_engine* e) {
    const auto num = env_num;
    e->opt_scan_dbg = (uint32_t)num("GFT_SCAN_DEBUG", 0);
    e->opt_scan_prio = num("GFT_SCAN_PRIO", 1) ? 1u : 0u;
    e->opt_scan_ordered = getenv("GFT_SCAN_ORDERED") ? 1u : 0u;
    e->opt_scan4_chunk = (uint32_t)num("GFT_SCAN4_CHUNK", 0);
    e->opt_scan4_round = (uint32_t)num("GFT_SCAN4_ROUND", 0);
    e->opt_solve.dbg = (uint32_t)num("GFT_SOLVE_DEBUG", 0);
    e->opt_solve.forced_group = (int)num("GFT_SOLVE_GROUP_DOCS", -1);
    e->opt_solve.prog_lds = num("GFT_SOLVE_PROG_LDS", 1) ? 1u : 0u;
}
// what plan_scan is told (table_set.hpp): GFT_SCAN_KERNEL and the GFT_SCAN5_* switches, read by gft_build / gft_import_tables
ScanOptions scan_options() {
    const auto num = env_num;
    ScanOptions o;
    o.forced = parse_forced(getenv("GFT_SCAN_KERNEL"));
    o.scan5_groups = (uint32_t)num("GFT_SCAN5_GROUPS", 0);
    o.scan5_large = num("GFT_SCAN5_LARGE", 1) ? 1u : 0u;
    o.scan5_bloom_kb = (uint32_t)std::min<long>(std::max<long>(num("GFT_SCAN5_BLOOM_KB", 32), 0), 64);
    o.scan5_fifo = (uint32_t)std::min<long>(std::max<long>(num("GFT_SCAN5_FIFO", 0), 0), 4096) & ~63u;
    return o;
}
#define GFT_LOCK(e) std::lock_guard<std::recursive_mutex> _gft_lock((e)->mu)

int fail(const gft_engine* e, int code, const std::string& msg) {
    e->err = msg;
    return code;
}
int fail_hip(const gft_engine* e, hipError_t h, const char* what) {
    e->err = std::string(what) + ": " + hipGetErrorString(h);
    return GFT_E_HIP;
}

#define HIP_TRY(expr, what)                                   \
    do {                                                      \
        hipError_t _h = (expr);                               \
        if (_h != hipSuccess) return fail_hip(e, _h, what);   \
    } while (0)

struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// Entry points that hand host memory (the caller's buffers, or temporaries of their own) to asynchronous copies: whatever
// path they leave by -- an error in the middle included -- the stream has drained before that memory can go away.
struct SyncOnExit {
    gft_engine* e;
    explicit SyncOnExit(gft_engine* e_) : e(e_) {}
    ~SyncOnExit() { if (e->device >= 0 && e->stream) (void)hipStreamSynchronize(e->stream); }
};

struct ProfScope {
    gft_engine* e;
    hipEvent_t a = nullptr, b = nullptr;
    ProfScope(gft_engine* e_, const char* cat) : e(e_) {
        if (!e->profiling || (e->profiling == 2 && std::strcmp(cat, "scan") != 0)) return;
        auto get = [&](hipEvent_t* ev) {
            if (!e->prof_pool.empty()) { *ev = e->prof_pool.back(); e->prof_pool.pop_back(); return true; }
            return hipEventCreate(ev) == hipSuccess;
        };
        if (!get(&a) || !get(&b)) { a = b = nullptr; return; }
        (void)hipEventRecord(a, e->stream);
        e->prof[cat].ev.emplace_back(a, b);
    }
    ~ProfScope() { if (b) (void)hipEventRecord(b, e->stream); }
};

template <class T>
int upload(gft_engine* e, DevBuf& buf, const std::vector<T>& v, const char* what) {
    HIP_TRY(buf.ensure(std::max<size_t>(v.size() * sizeof(T), 16)), what);
    if (!v.empty()) HIP_TRY(hipMemcpyAsync(buf.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, e->stream), what);
    return GFT_OK;
}

int ensure_pool(gft_engine* e, uint64_t entries) {
    if (entries <= e->pool_cap) return GFT_OK;
    HIP_TRY(e->d_pool_term.ensure(entries * 4), "pool alloc");
    HIP_TRY(e->d_pool_pos.ensure(entries * 4), "pool alloc");
    e->pool_cap = std::min(e->d_pool_term.cap, e->d_pool_pos.cap) / 4;
    return GFT_OK;
}

// slabs of the last completed scan -> canonical CSR in e->d_match_off / d_term / d_pos (document order, the reference's
// emission order inside a document).  The unit table, the slabs and the counts of that scan are still in the engine
// (e->pool); positions must have been written (want_pos).
int csr_from_pool(gft_engine* e, uint64_t n_docs) {
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
uint64_t grid_waves(const gft_engine* e, uint64_t work) {
    const uint64_t wpw = e->plan.scan_waves;
    return std::min<uint64_t>(std::max<uint64_t>((work + wpw - 1) / wpw, 1), e->n_cus) * wpw;
}
// the smallest slab of scan2 / scan3 / scan5 (scan4 sizes its slabs from a chunk's need)
constexpr uint64_t slab_floor(ScanKernel k) { return k == ScanKernel::scan3 ? 2 * kScan3MinRoom : 64; }
// ... and their slab: the slack is at most one slab per resident wave, keep it below half the pool
uint32_t slab_size(const gft_engine* e) {
    const uint64_t n_waves = (uint64_t)e->n_cus * e->plan.scan_waves;
    return (uint32_t)std::min<uint64_t>(kScan2Slab, std::max<uint64_t>(slab_floor(e->plan.kernel), e->pool_cap / (2 * n_waves)));
}

ScanParams dfa_params(const gft_engine* e, const ScanBatch& b) {
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

Scan3Params scan3_params(const gft_engine* e, const ScanBatch& b) {
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
Scan2Params scan2_params(const gft_engine* e, const ScanBatch& b) {
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
int enqueue_scan(gft_engine* e, const ScanBatch& b, ScanLaunch& L) {
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
void learn_from_batch(gft_engine* e, const ScanLaunch& L, const BatchVerdict& v) {
    const ScanKernel k = e->plan.kernel;
    learn(e->learned, k, k == ScanKernel::scan5 ? e->plan.s5plan.fifo_cap : kScan2FifoCap, L.ordered, v.total, v.text_lo, v.text_hi);
}

// The device pipeline shared by scan and process.  On success the canonical CSR sits in e->d_match_off / d_term / d_pos
// (need_csr) and `v` says what the scan established -- unless the launch was deferred: deferred_interpret then does.
constexpr uint64_t kHostUnitDocs = 1024;   // batches up to this many documents get their unit table from the host

// defer != nullptr: the launch may be deferred -- the caller reads the control block back itself after its last kernel
// (deferred_interpret), the unit table and the match pool are sized from the previous batch, and a batch that outgrew them is
// run again.  *defer says whether it was, and what the launch knew.
int scan_pipeline(gft_engine* e, const uint8_t* d_text, const uint64_t* d_doc_off, uint64_t n_docs, uint32_t flags,
                  bool need_csr, BatchVerdict& v, const uint64_t* h_doc_off = nullptr, ScanLaunch* defer = nullptr) {
    hipStream_t st = e->stream;
    v = BatchVerdict();                   // (an empty batch: nothing scanned, no range for refine_nonascii to judge)
    ScanLaunch L;
    if (defer) *defer = L;
    e->pool = PoolState();                // the pool is about to be overwritten
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

    // 1. work units
    HIP_TRY(e->d_ctl.ensure(kCtlBytes), "control alloc");
    HIP_TRY(e->d_unit_cnt.ensure(n_docs * 4), "unit alloc");
    HIP_TRY(e->d_unit_base.ensure((n_docs + 1) * 8), "unit alloc");
    HIP_TRY(e->d_partial.ensure(scan_partials_needed(n_docs) * 8), "unit alloc");
    uint64_t n_units = 0, text_lo = 0, text_hi = 0;
    // small batches from host memory (a single ProcessText / FindSubstrings call is the reference's own shape): the unit
    // table is a few entries, computed here and uploaded instead of five kernel launches and a synchronising read-back
    const bool host_units = h_doc_off != nullptr && n_docs <= kHostUnitDocs;
    // The batch before was one unit per document: this one gets its unit table from ONE launch on that assumption
    // (k_units_single) instead of count + prefix sum + fill + clamp; deferred_interpret learns whether it held.  That launch
    // also clears the control block (its two flags are raised to the batch's EPOCH, a number no earlier batch wrote there,
    // so they need no clearing): one node less on the stream of every batch
    const uint64_t cap_units = std::min(std::min(e->d_units.cap / sizeof(Unit), e->d_unit_start.cap / 8), e->d_unit_count.cap / 4);
    bool units_single = !host_units && defer && !need_csr && e->learned.single_streak >= 2 && e->pool_cap > 0 && cap_units >= n_docs;
    if (units_single && ++e->ctl_epoch < 2) { e->ctl_epoch = 1; units_single = false; }      // (wrapped: this batch the general way)
    if (!units_single) HIP_TRY(hipMemsetAsync(e->d_ctl.p, 0, kCtlBatchClear, st), "memset");
    std::vector<uint64_t> hub;
    std::vector<Unit> hun;
    struct DrainIf { gft_engine* e; bool on; ~DrainIf() { if (on && e->stream) (void)hipStreamSynchronize(e->stream); } } drain_units{e, host_units};
    if (host_units) {
        hub.assign(n_docs + 1, 0);
        for (uint64_t d = 0; d < n_docs; d++) {
            if (h_doc_off[d + 1] < h_doc_off[d]) return fail(e, GFT_E_INVALID, "doc_off is not ascending");
            const uint64_t n = h_doc_off[d + 1] - h_doc_off[d];
            if (n > 0xFFFFFFFFull) return fail(e, GFT_E_UNSUPPORTED, "a document is longer than 4 GiB - 1 bytes (positions are 32-bit)");
            const uint64_t k = n <= unit_max ? 1 : (n + unit_max - 1) / unit_max;
            hub[d + 1] = hub[d] + k;
            const uint64_t per = (n + k - 1) / k;                 // as k_unit_fill
            for (uint64_t i = 0; i < k; i++) {
                uint64_t lo = i * per, hi = lo + per < n ? lo + per : n;
                if (lo > n) lo = n;
                hun.push_back(Unit{(uint32_t)d, (uint32_t)lo, (uint32_t)hi});
            }
        }
        n_units = hub[n_docs]; text_lo = h_doc_off[0]; text_hi = h_doc_off[n_docs];
        HIP_TRY(hipMemcpyAsync(e->d_unit_base.p, hub.data(), (n_docs + 1) * 8, hipMemcpyHostToDevice, st), "unit upload");
    } else if (units_single) {
        ProfScope ps(e, "aux");
        HIP_TRY(launch_units_single(d_doc_off, n_docs, unit_max, e->d_units.as<Unit>(), e->d_unit_base.as<uint64_t>(),
                                    ctl_at<uint32_t>(e, kCtlBad), e->ctl_epoch, st), "unit table");
        n_units = n_docs; text_lo = 0; text_hi = ~0ull;
        L.deferred = L.single = true; L.epoch = e->ctl_epoch;
        L.unit_cap = L.n_docs = n_docs;
    } else {
        {
            ProfScope ps(e, "aux");
            HIP_TRY(launch_unit_count(d_doc_off, n_docs, unit_max, e->d_unit_cnt.as<uint32_t>(), ctl_at<uint32_t>(e, kCtlBad), st), "unit_count");
            HIP_TRY(launch_exclusive_scan(e->d_unit_cnt.as<uint32_t>(), n_docs, e->d_unit_base.as<uint64_t>(),
                                          e->d_partial.as<uint64_t>(), st), "unit scan");
            HIP_TRY(launch_pack_ctl(e->d_unit_base.as<uint64_t>(), d_doc_off, n_docs, ctl_at<uint64_t>(e, kCtlUnits), st), "unit scan");
        }
        // No read-back when the caller checks afterwards: the tables keep the size the last batch gave them (a document
        // is one unit unless it is longer than unit_max), units beyond the table are dropped and every index is clamped
        // into it -- deferred_interpret sees the true count and has the batch run again
        L.deferred = defer && !need_csr && cap_units >= n_docs && e->pool_cap > 0;
        if (L.deferred) {
            n_units = cap_units; text_lo = 0; text_hi = ~0ull;       // (the text blob is readable 64 bytes past its end: gft.h)
            L.unit_cap = cap_units; L.n_docs = n_docs;
        } else {
            uint64_t raw[kCtlWords] = {};
            HIP_TRY(hipMemcpyAsync(raw, e->d_ctl.p, sizeof raw, hipMemcpyDeviceToHost, st), "readback");
            HIP_TRY(hipStreamSynchronize(st), "sync");
            const CtlBlock c = decode_ctl(raw);
            n_units = c.n_units; text_lo = c.text_lo; text_hi = c.text_hi;
            count_streak(e->learned, n_units, n_docs);
            if (text_hi < text_lo) return fail(e, GFT_E_INVALID, "doc_off is not ascending");
            if (c.bad) return fail(e, GFT_E_INVALID, "doc_off is not ascending, or a document is longer than 4 GiB - 1 bytes (positions are 32-bit)");
        }
    }

    if (!L.deferred) { v.text_lo = text_lo; v.text_hi = text_hi; }
    HIP_TRY(e->d_units.ensure(n_units * sizeof(Unit)), "unit alloc");
    HIP_TRY(e->d_unit_start.ensure(n_units * 8), "unit alloc");
    HIP_TRY(e->d_unit_count.ensure(n_units * 4), "unit alloc");
    HIP_TRY(e->d_unit_out.ensure((n_units + 1) * 8), "unit alloc");
    HIP_TRY(e->d_partial.ensure(scan_partials_needed(std::max(n_units, n_docs)) * 8), "unit alloc");
    {
        ProfScope ps(e, "aux");
        if (host_units) {
            if (n_units) HIP_TRY(hipMemcpyAsync(e->d_units.p, hun.data(), n_units * sizeof(Unit), hipMemcpyHostToDevice, st), "unit upload");
        } else if (L.single) {
            // (k_units_single has filled the table)
        } else if (L.deferred) {
            HIP_TRY(hipMemsetAsync(e->d_units.p, 0, n_units * sizeof(Unit), st), "memset");      // empty units behind the real ones
            HIP_TRY(launch_unit_fill(d_doc_off, n_docs, e->d_unit_base.as<uint64_t>(), e->d_units.as<Unit>(), unit_max, st, n_units), "unit_fill");
            HIP_TRY(launch_clamp_u64(e->d_unit_base.as<uint64_t>(), n_docs + 1, n_units, st), "unit clamp");
        } else {
            HIP_TRY(launch_unit_fill(d_doc_off, n_docs, e->d_unit_base.as<uint64_t>(), e->d_units.as<Unit>(), unit_max, st), "unit_fill");
        }
    }

    // 2. automaton walk into the slab pool; grow the pool and re-run if it overflowed (never truncate)
    const ScanKernel k = e->plan.kernel;
    if (L.deferred) L.pool_cap = e->pool_cap;
    int rc = L.deferred ? GFT_OK : ensure_pool(e, std::max<uint64_t>(1u << 20, (text_hi - text_lo) / 16));
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

// gft_process_device_begin / _end: no batch in flight is still to be completed (the synchronous entry points may run)
bool pend_settled(const gft_engine* e) {
    for (unsigned i = 0; i < e->pend_count; i++)
        if (!e->pend[(e->pend_head + i) % 2].done) return false;
    return true;
}

// GFT_SCAN_UNIQUE: the canonical CSR in d_match_off / d_term -> every term once per document, first occurrences in order.
// The result replaces d_match_off / d_term (positions: zeros in d_pos); *n_matches = new total.
int unique_pipeline(gft_engine* e, uint64_t n_docs, uint64_t* n_matches) {
    if (!n_docs) return GFT_OK;
    hipStream_t st = e->stream;
    const uint32_t n_terms = std::max<uint32_t>((uint32_t)e->tables.tab.terms.size(), 1);
    // as many workgroups as 256 MB of first-occurrence rows allow, at most 4 per CU
    const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(n_docs, (uint64_t)e->n_cus * 4), (256ull << 20) / ((uint64_t)n_terms * 4)));
    HIP_TRY(e->d_uq_first.ensure((size_t)grid * n_terms * 4), "unique alloc");
    HIP_TRY(e->d_uq_cnt.ensure(n_docs * 4), "unique alloc");
    HIP_TRY(e->d_uq_off.ensure((n_docs + 1) * 8), "unique alloc");
    HIP_TRY(e->d_partial.ensure(scan_partials_needed(n_docs) * 8), "unique alloc");
    HIP_TRY(hipMemsetAsync(e->d_uq_first.p, 0xFF, (size_t)grid * n_terms * 4, st), "memset");
    ProfScope ps(e, "aux");
    HIP_TRY(launch_unique_terms(false, e->d_match_off.as<uint64_t>(), e->d_term.as<uint32_t>(), n_docs, n_terms, e->d_uq_first.as<uint32_t>(), grid,
                                e->d_uq_cnt.as<uint32_t>(), nullptr, nullptr, st), "unique count");
    HIP_TRY(launch_exclusive_scan(e->d_uq_cnt.as<uint32_t>(), n_docs, e->d_uq_off.as<uint64_t>(), e->d_partial.as<uint64_t>(), st), "unique scan");
    uint64_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, e->d_uq_off.as<uint64_t>() + n_docs, 8, hipMemcpyDeviceToHost, st), "readback");
    HIP_TRY(hipStreamSynchronize(st), "unique scan");
    HIP_TRY(e->d_uq_term.ensure(std::max<uint64_t>(total, 1) * 4), "unique alloc");
    HIP_TRY(launch_unique_terms(true, e->d_match_off.as<uint64_t>(), e->d_term.as<uint32_t>(), n_docs, n_terms, e->d_uq_first.as<uint32_t>(), grid,
                                nullptr, e->d_uq_off.as<uint64_t>(), e->d_uq_term.as<uint32_t>(), st), "unique write");
    // the caller-visible buffers: offsets and terms are swapped in, positions are all zero (substringEngine.go:83)
    std::swap(e->d_match_off, e->d_uq_off);
    std::swap(e->d_term, e->d_uq_term);
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
    HIP_TRY(e->d_rn_cnt.ensure(n_docs * 4), "rune alloc");
    HIP_TRY(e->d_rn_base.ensure((n_docs + 1) * 8), "rune alloc");
    HIP_TRY(e->d_partial.ensure(scan_partials_needed(n_docs) * 8), "rune alloc");
    ProfScope ps(e, "aux");
    HIP_TRY(launch_rune_doc_blocks(d_doc_off, n_docs, e->d_rn_cnt.as<uint32_t>(), st), "rune blocks");
    HIP_TRY(launch_exclusive_scan(e->d_rn_cnt.as<uint32_t>(), n_docs, e->d_rn_base.as<uint64_t>(), e->d_partial.as<uint64_t>(), st), "rune scan");
    uint64_t n_blocks = 0;
    HIP_TRY(hipMemcpyAsync(&n_blocks, e->d_rn_base.as<uint64_t>() + n_docs, 8, hipMemcpyDeviceToHost, st), "readback");
    HIP_TRY(hipStreamSynchronize(st), "rune scan");
    HIP_TRY(e->d_rn_starts.ensure(std::max<uint64_t>(n_blocks, 1) * 4), "rune alloc");
    HIP_TRY(e->d_rn_prefix.ensure((n_blocks + 1) * 8), "rune alloc");
    HIP_TRY(e->d_partial.ensure(scan_partials_needed(std::max(n_blocks, n_docs)) * 8), "rune alloc");
    HIP_TRY(launch_rune_block_starts(d_text, d_doc_off, e->d_rn_base.as<uint64_t>(), n_docs, n_blocks, e->d_rn_starts.as<uint32_t>(), st), "rune starts");
    HIP_TRY(launch_exclusive_scan(e->d_rn_starts.as<uint32_t>(), n_blocks, e->d_rn_prefix.as<uint64_t>(), e->d_partial.as<uint64_t>(), st), "rune scan");
    HIP_TRY(launch_pos_to_rune(d_text, d_doc_off, e->d_rn_base.as<uint64_t>(), e->d_rn_prefix.as<uint64_t>(), e->d_match_off.as<uint64_t>(), n_docs,
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
    const SolvePlan plan = plan_solve(shape, e->lds_max, e->n_cus, n_docs, e->opt_solve);
    S.tile_words = plan.tile_words;
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
struct HostPlan {
    bool all_docs = false;                     // some expression is beyond the device solver's limits: every document
    std::vector<uint64_t> irregular;           // documents in which a slot read by an INORD group may have a non-ascending list
    bool empty() const { return !all_docs && irregular.empty(); }
};

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

}  // namespace

namespace {
void destroy_multi(gft_engine* e);
// multi-device dispatch (definitions behind the single-device entry points)
int multi_process(gft_engine* e, const uint8_t* text_blob, const uint64_t* doc_off, uint64_t n_docs, uint32_t flags,
                  const gft_extra_matches* extra, uint32_t* hit_bitmap);
int multi_process_again(gft_engine* e, uint64_t n_docs, const gft_extra_matches* extra, uint32_t* hit_bitmap);
int multi_scan(gft_engine* e, const uint8_t* text_blob, const uint64_t* doc_off, uint64_t n_docs, uint32_t flags, gft_matches* out);
int multi_set_programs(gft_engine* e, const uint32_t* prog_words, const uint64_t* prog_off, uint32_t n_exprs, uint32_t n_extra);
int multi_build(gft_engine* e, const uint8_t* terms_blob, const uint64_t* term_off, uint32_t n_terms, uint32_t flags);
int multi_import_tables(gft_engine* e, const uint8_t* blob, uint64_t len);

}  // namespace


extern "C" {

int gft_engine_create(gft_engine** out, int device) try {
    if (!out) return GFT_E_INVALID;
    *out = nullptr;
    std::unique_ptr<gft_engine> owner(new gft_engine());     // (released into *out on every regular way out)
    gft_engine* e = owner.get();
    int count = 0;
    hipError_t h = hipGetDeviceCount(&count);
    if (h != hipSuccess || count == 0) {
        // keep the handle so the caller can read the message, but every compute call will fail loudly
        e->device = -1;
        e->err = std::string("no HIP device available: ") + (h != hipSuccess ? hipGetErrorString(h) : "device count is 0");
        *out = owner.release();
        return GFT_E_HIP;
    }
    if (device < 0) { if (hipGetDevice(&device) != hipSuccess) device = 0; }
    e->device = device;
    DeviceGuard g(device);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) {
        e->n_cus_hw = prop.multiProcessorCount > 0 ? (unsigned)prop.multiProcessorCount : 256;
        if (const char* m = getenv("GFT_CU_MARGIN")) { const int v = atoi(m); if (v > 0) e->cu_margin = (unsigned)v; }
        e->n_cus = e->n_cus_hw > e->cu_margin ? e->n_cus_hw - e->cu_margin : 1;
        int optin = 0;
        if (hipDeviceGetAttribute(&optin, hipDeviceAttributeSharedMemPerBlockOptin, device) != hipSuccess) optin = 0;
        e->lds_max = std::max<size_t>(prop.sharedMemPerBlock, (size_t)std::max(optin, 0));
        if (std::string(prop.gcnArchName).find("gfx950") != std::string::npos) e->lds_max = std::max<size_t>(e->lds_max, 160 * 1024);
    }
    // a blocking stream: ordered with the legacy default stream, which is where a caller that never names a stream
    // (torch's default stream, plain hipMemcpy) produces the device buffers it hands to *_device entry points
    if (hipStreamCreateWithFlags(&e->stream, hipStreamDefault) == hipSuccess) e->own_stream = true;
    else e->stream = nullptr;
    refresh_options(e);
    *out = owner.release();
    return GFT_OK;
} GFT_CATCH(nullptr)

void gft_engine_destroy(gft_engine* e) {
    if (!e) return;
    destroy_multi(e);
    if (e->device >= 0) {
        DeviceGuard g(e->device);
        if (e->stream) (void)hipStreamSynchronize(e->stream);
        for (auto& kv : e->prof)
            for (auto& p : kv.second.ev) { e->prof_pool.push_back(p.first); e->prof_pool.push_back(p.second); }
        for (hipEvent_t ev : e->prof_pool) (void)hipEventDestroy(ev);
        gft_engine::TableBufs& t = e->d_tabs;
        DevBuf* all[] = {&t.dfa.byte_class, &t.dfa.delta, &t.dfa.out_term, &t.dfa.out_link, &t.dfa.term_len, &e->d_progs.prog,
                         &e->d_progs.prog_off, &e->d_progs.fprog, &e->d_progs.fprog_off, &e->d_progs.groups, &e->d_progs.order, &e->d_progs.blk_class, &e->d_progs.wave_blk,
                         &e->d_progs.fprog_t, &e->d_progs.fblk_off, &e->d_progs.wide_list, &e->d_wide_slot, &e->d_wide_theta, &e->d_pscratch, &e->d_solve_dbg, &t.s2.filter,
                         &t.s2.slots, &t.s2.more, &t.s2.cls, &t.s2.cls_fold, &t.s2.term_blob,
                         &t.s2.term_off, &e->d_ctl, &e->d_dbg, &t.s2.short3, &t.s2.shorts_packed, &t.s2.short3_big, &t.s2.fpt,
                         &t.s3.filter, &t.s3.short3, &t.s3.srec, &t.s3.short3_big, &t.s3.srec_big, &t.s3.bloom, &t.s3.slots,
                         &t.s3.more, &t.s3.cls, &t.s3.cls_fold, &t.s3.term_blob, &t.s3.term_off,
                         &t.s5.grp, &t.s5.grp_fold, &t.s5.filter, &t.s5.bloom,
                         &e->d_unit_cnt, &e->d_unit_base, &e->d_units, &e->d_partial,
                         &e->d_pool_term, &e->d_pool_pos, &e->d_unit_start, &e->d_unit_count, &e->d_unit_out,
                         &e->d_term, &e->d_pos, &e->d_match_off, &e->d_text, &e->d_doc_off, &e->d_bitmap, &e->d_xoff,
                         &e->d_xslot, &e->d_xpos, &e->d_uq_first, &e->d_uq_cnt, &e->d_uq_off, &e->d_uq_term, &e->d_patch, &e->d_rn_cnt, &e->d_rn_base, &e->d_rn_starts, &e->d_rn_prefix,
                         &e->d_labels, &e->d_cp_cnt, &e->d_cp_partial, &e->d_cp_row_off, &e->d_cp_idx, &e->d_cp_label,
                         &e->d_lw_page, &e->d_lw_delta, &e->d_lw_doc_units, &e->d_lw_unit_base, &e->d_lw_units, &e->d_lw_partial,
                         &e->d_lw_unit_cnt, &e->d_lw_unit_out, &e->d_lw_ctl, &e->d_lw_text, &e->d_lw_off};
        for (DevBuf* b : all) b->release();
        gft_engine::RuleBufs& rb = e->d_rules;
        for (DevBuf* b : {&rb.expr_tag, &rb.masks, &rb.units, &rb.prog, &rb.prog_off, &rb.leaf_bitmap, &rb.tag_rows, &rb.flags}) b->release();
        for (DevBuf& b : rb.stage) b.release();
        for (int k = 0; k < 2; k++) {
            if (e->pin[k]) (void)hipHostFree(e->pin[k]);
            if (k == 0 && e->pin_rb) (void)hipHostFree(e->pin_rb);
            if (e->pin_ev[k]) (void)hipEventDestroy(e->pin_ev[k]);
            if (e->pend[k].rb) (void)hipHostFree(e->pend[k].rb);
            if (e->pend[k].ev) (void)hipEventDestroy(e->pend[k].ev);
        }
        if (e->own_stream && e->stream) (void)hipStreamDestroy(e->stream);
    }
    delete e;
}

const char* gft_last_error(const gft_engine* e) { return e ? e->err.c_str() : "null engine"; }

int gft_set_stream(gft_engine* e, void* hip_stream) try {
    if (!e) return GFT_E_INVALID;
    GFT_LOCK(e);
    if (e->device < 0) return fail(e, GFT_E_HIP, "no HIP device available");
    DeviceGuard g(e->device);
    if (e->own_stream && e->stream) { (void)hipStreamSynchronize(e->stream); (void)hipStreamDestroy(e->stream); }
    e->own_stream = false;
    e->stream = (hipStream_t)hip_stream;
    if (!hip_stream) {
        HIP_TRY(hipStreamCreateWithFlags(&e->stream, hipStreamDefault), "stream create");
        e->own_stream = true;
    }
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))


int gft_set_cu_margin(gft_engine* e, uint32_t margin) try {
    if (!e) return GFT_E_INVALID;
    GFT_LOCK(e);
    if (e->device < 0) return fail(e, GFT_E_HIP, "no HIP device available");
    if (e->pend_count) return fail(e, GFT_E_INVALID, "batches are in flight (gft_process_device_end first)");
    e->cu_margin = margin;
    e->n_cus = e->n_cus_hw > margin ? e->n_cus_hw - margin : 1;
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

// scan3's short-term tables, which scan5 reads too over an alphabet too large for scan2's
static int upload_scan3_short_tables(gft_engine* e, const Scan3Tables& s3) {
    const std::vector<uint8_t> none(16, 0), g1(s3.cls, s3.cls + 256), g2(s3.cls_fold, s3.cls_fold + 256);
    SyncOnExit drained(e);                              // (the uploads read from these locals)
    auto& d = e->d_tabs.s3;
    int rc;
    if ((rc = upload(e, d.short3, s3.short3.empty() ? none : s3.short3, "table upload"))) return rc;
    if ((rc = upload(e, d.srec, s3.srec, "table upload"))) return rc;
    if (!s3.short3_big.empty() && (rc = upload(e, d.short3_big, s3.short3_big, "table upload"))) return rc;
    if ((rc = upload(e, d.srec_big, s3.srec_big, "table upload"))) return rc;
    if ((rc = upload(e, d.cls, g1, "table upload"))) return rc;
    if ((rc = upload(e, d.cls_fold, g2, "table upload"))) return rc;
    return GFT_OK;
}

// Installs a compiled set (gft_build's, gft_import_tables', or a copy of the first device's): chooses the scan kernel for
// this device, derives what it needs on top, uploads what it reads -- all from `set`, which nothing edits -- and commits.
// A refusal comes before the first upload and leaves the handle as it was; from the first upload until the last has landed
// the handle is not built, so an upload error gives GFT_E_NOT_BUILT and never a mixture of two dictionaries.
static int install_tables(gft_engine* e, TableSet&& set, uint32_t flags) {
    const AcTables& tab = set.tab;
    const Scan2Tables& s2 = set.s2;
    const Scan3Tables& s3 = set.s3;
    ScanPlan plan;
    int rc = plan_scan(set, scan_options(), e->lds_max, kExtraKernels, plan, e->err);
    if (rc) return rc;
    const ScanKernel k = plan.kernel;
    Scan5Tables s5;
    std::vector<uint32_t> s5_bloom;
    if (k == ScanKernel::scan5) derive_scan5(set, plan, s5, s5_bloom);
    const bool build_dbg = getenv("GFT_SCAN_DEBUG") != nullptr;
    if (build_dbg && k == ScanKernel::scan3)
        fprintf(stderr, "[gft build debug] scan3: G=%u%s keys=%llu anchors=%llu slots=%zu more=%zu bloom 2^%u (%s) short cells: lds records %zu, big words %zu; waves=%u cand_cap=%u\n",
                s3.G, s3.grouped ? " (merged classes)" : "", (unsigned long long)s3.n_keys, (unsigned long long)s3.n_anchors,
                s3.slots.size(), s3.more.size(), s3.bloom_lg, s3.bloom_lg <= kScan3BloomLdsLg ? "LDS" : "global", s3.srec.size() / kScan3RecWords - 1,
                s3.srec_big.size(), plan.scan_waves, plan.scan3_cand_cap);
    if (build_dbg && on_scan2_tables(k)) {
        size_t n_ff = 0, n_used = 0, n_simple = 0, n_slots = 0;
        for (uint8_t b : s2.fpt) { n_ff += b == 0xFF; n_used += b != 0; }
        for (const auto& s : s2.slots) { n_slots += s.key != kScan2EmptyKey; n_simple += s.key != kScan2EmptyKey && !(s.info & kScan2Multi); }
        fprintf(stderr, "[gft build debug] kp=%u keys=%zu (simple %zu) slots=%zu fpt: used=%zu always-pass=%zu of %u; shorts=%zu filter=%s %u bits waves=%u\n",
                s2.kp, n_slots, n_simple, s2.slots.size(), n_used, n_ff, (unsigned)s2.fpt.size(), s2.shorts.size() - 1,
                s2.hashed ? "hashed" : "direct", s2.filter_bits, plan.scan_waves);
        fprintf(stderr, "[gft build debug] candidate list capacity %u per wave\n", k == ScanKernel::scan5 ? plan.s5plan.cand_cap : plan.scan2_cand_cap);
    }
    if (build_dbg && k == ScanKernel::scan5) {
        size_t set_bits = 0;
        for (uint32_t w : s5_bloom) set_bits += (size_t)__builtin_popcount(w);
        fprintf(stderr, "[gft build debug] scan5: G=%u of %u classes, filter %zu entries, list %u, term bits %u; Bloom level 2^%u bits, %.1f %% set\n",
                s5.G, s2.kp, s5.filter.size(), plan.s5plan.cand_cap, plan.s5_term_bits, plan.s5_bloom_lg,
                plan.s5_bloom_lg ? 100.0 * (double)set_bits / (double)(1ull << plan.s5_bloom_lg) : 0.0);
    }

    refresh_options(e);
    DeviceGuard g(e->device);
    // (an empty short3 is uploaded as 16 zero bytes; the kernel is told 0 bytes)
    const std::vector<uint8_t> none(16, 0), bc(tab.byte_class, tab.byte_class + 256), c1(s2.cls, s2.cls + 256), c2(s2.cls_fold, s2.cls_fold + 256);
    std::vector<uint8_t> s5g, s5gf;
    if (k == ScanKernel::scan5) { s5g.assign(s5.grp, s5.grp + 256); s5gf.assign(s5.grp_fold, s5.grp_fold + 256); }
    SyncOnExit drained(e);                              // (declared behind the temporaries the uploads read from: it goes first)
    e->built = false;
    e->have_programs = false;   // slots refer to the dictionary: programs must be set again
    e->n_exprs = 0;
    gft_engine::TableBufs& d = e->d_tabs;
    if ((rc = upload(e, d.dfa.byte_class, bc, "table upload"))) return rc;
    if ((rc = upload(e, d.dfa.delta, tab.delta, "table upload"))) return rc;
    if ((rc = upload(e, d.dfa.out_term, tab.out_term, "table upload"))) return rc;
    if ((rc = upload(e, d.dfa.out_link, tab.out_link, "table upload"))) return rc;
    if ((rc = upload(e, d.dfa.term_len, tab.term_len, "table upload"))) return rc;
    if (k == ScanKernel::scan3) {
        if ((rc = upload_scan3_short_tables(e, s3))) return rc;
        if ((rc = upload(e, d.s3.filter, s3.filter, "table upload"))) return rc;
        if ((rc = upload(e, d.s3.bloom, s3.bloom, "table upload"))) return rc;
        if ((rc = upload(e, d.s3.slots, s3.slots, "table upload"))) return rc;
        if ((rc = upload(e, d.s3.more, s3.more, "table upload"))) return rc;
        if ((rc = upload(e, d.s3.term_blob, s3.term_blob, "table upload"))) return rc;
        if ((rc = upload(e, d.s3.term_off, s3.term_off, "table upload"))) return rc;
    }
    if (on_scan2_tables(k)) {
        if (k == ScanKernel::scan5 && plan.s5_short_groups && (rc = upload_scan3_short_tables(e, s3))) return rc;
        if ((rc = upload(e, d.s2.short3, s2.short3.empty() ? none : s2.short3, "table upload"))) return rc;
        if ((rc = upload(e, d.s2.shorts_packed, s2.shorts_packed, "table upload"))) return rc;
        if (!s2.short3_big.empty() && (rc = upload(e, d.s2.short3_big, s2.short3_big, "table upload"))) return rc;
        if ((rc = upload(e, d.s2.fpt, s2.fpt, "table upload"))) return rc;
        if ((rc = upload(e, d.s2.cls, c1, "table upload"))) return rc;
        if ((rc = upload(e, d.s2.cls_fold, c2, "table upload"))) return rc;
        if ((rc = upload(e, d.s2.filter, s2.filter, "table upload"))) return rc;
        if ((rc = upload(e, d.s2.slots, s2.slots, "table upload"))) return rc;
        if ((rc = upload(e, d.s2.more, s2.more, "table upload"))) return rc;
        if ((rc = upload(e, d.s2.term_blob, s2.term_blob, "table upload"))) return rc;
        if ((rc = upload(e, d.s2.term_off, s2.term_off, "table upload"))) return rc;
    }
    if (k == ScanKernel::scan5) {
        if ((rc = upload(e, d.s5.grp, s5g, "table upload"))) return rc;
        if ((rc = upload(e, d.s5.grp_fold, s5gf, "table upload"))) return rc;
        if ((rc = upload(e, d.s5.filter, s5.filter, "table upload"))) return rc;
        if (plan.s5_bloom_lg && (rc = upload(e, d.s5.bloom, s5_bloom, "table upload"))) return rc;
    }
    HIP_TRY(hipStreamSynchronize(e->stream), "table upload");
    e->tables = std::move(set);
    e->plan = plan;
    e->s5 = std::move(s5);
    e->build_flags = flags;
    e->pool.valid_docs = ~0ull;
    e->learned.unit_max = kScan2UnitMax;
    e->learned.scan4_density = 0.06;
    e->built = true;
    return GFT_OK;
}


int gft_build(gft_engine* e, const uint8_t* terms_blob, const uint64_t* term_off, uint32_t n_terms, uint32_t flags) try {
    if (!e || (n_terms && (!terms_blob || !term_off))) return e ? fail(e, GFT_E_INVALID, "null argument") : GFT_E_INVALID;
    GFT_LOCK(e);
    if (!e->peers.empty() && !e->in_multi) return multi_build(e, terms_blob, term_off, n_terms, flags);
    if (e->device < 0) return fail(e, GFT_E_HIP, "no HIP device available");
    std::vector<std::string> terms;
    terms.reserve(n_terms);
    for (uint32_t i = 0; i < n_terms; i++) {
        if (term_off[i + 1] < term_off[i]) return fail(e, GFT_E_INVALID, "term_off is not ascending");
        terms.emplace_back((const char*)terms_blob + term_off[i], (size_t)(term_off[i + 1] - term_off[i]));
    }
    TableSet set;
    compile_tables(std::move(terms), set);
    return install_tables(e, std::move(set), flags);
} GFT_CATCH((e ? &e->err : nullptr))

uint32_t gft_n_terms(const gft_engine* e) { return e ? (uint32_t)e->tables.tab.terms.size() : 0; }
uint32_t gft_n_states(const gft_engine* e) { return e ? e->tables.tab.n_states : 0; }
uint32_t gft_n_exprs(const gft_engine* e) { return e ? e->n_exprs : 0; }
uint32_t gft_n_host_exprs(const gft_engine* e) { return e ? (uint32_t)e->progs.host_only.size() : 0; }
int gft_last_nonascii(const gft_engine* e) { return e && e->reported.nonascii ? 1 : 0; }
const char* gft_build_info(void) { return kExtraKernels ? "gfx950 extra_kernels=1" : "gfx950 extra_kernels=0"; }
const char* gft_scan_kernel(const gft_engine* e) {
    if (!e || !e->built) return "";
    return kScanKernelName[(int)e->plan.kernel];
}

int gft_term(const gft_engine* e, uint32_t term_id, const uint8_t** ptr, uint32_t* len) try {
    if (!e || !ptr || !len) return GFT_E_INVALID;
    if (term_id >= e->tables.tab.terms.size()) return fail(e, GFT_E_INVALID, "term id out of range");
    *ptr = (const uint8_t*)e->tables.tab.terms[term_id].data();
    *len = (uint32_t)e->tables.tab.terms[term_id].size();
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

int64_t gft_term_id(const gft_engine* e, const uint8_t* term, uint32_t len) try {
    if (!e) return -1;
    std::string s((const char*)term, len);
    auto it = std::lower_bound(e->tables.tab.terms.begin(), e->tables.tab.terms.end(), s);
    if (it == e->tables.tab.terms.end() || *it != s) return -1;
    return (int64_t)(it - e->tables.tab.terms.begin());
} GFT_CATCH_VALUE(-1)


int gft_export_tables(const gft_engine* e, uint8_t* out, uint64_t cap, uint64_t* needed) try {
    if (!e) return GFT_E_INVALID;
    GFT_LOCK(e);
    if (!e->built) return fail(e, GFT_E_NOT_BUILT, "gft_build has not been called");
    std::vector<uint8_t> b;
    write_tables(e->tables, e->build_flags, b);
    if (needed) *needed = b.size();
    if (!out || cap < b.size()) return GFT_E_INVALID;
    memcpy(out, b.data(), b.size());
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

int gft_import_tables(gft_engine* e, const uint8_t* blob, uint64_t len) try {
    if (!e || !blob) return e ? fail(e, GFT_E_INVALID, "null argument") : GFT_E_INVALID;
    GFT_LOCK(e);
    if (!e->peers.empty() && !e->in_multi) return multi_import_tables(e, blob, len);
    TableSet set;
    uint32_t flags = 0;
    const int rc = read_tables(blob, len, set, flags, e->err);
    if (rc) return rc;          // the handle is untouched: the dictionary installed before, if any, still is
    if (e->device < 0) return fail(e, GFT_E_HIP, "no HIP device available");
    return install_tables(e, std::move(set), flags);
} GFT_CATCH((e ? &e->err : nullptr))

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

// a scan entry point's last act on every way out behind its scan: the batch's verdict becomes the handle's
struct Publish {
    gft_engine* e; const BatchVerdict& v;
    ~Publish() { e->reported = v; }
};

int gft_scan_device(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs,
                    uint32_t flags, gft_matches* out_dev) try {
    if (!e || !out_dev || (n_docs && (!d_text_blob || !d_doc_off))) return e ? fail(e, GFT_E_INVALID, "null argument") : GFT_E_INVALID;
    GFT_LOCK(e);
    if (e->device < 0) return fail(e, GFT_E_HIP, "no HIP device available");
    if (!e->built) return fail(e, GFT_E_NOT_BUILT, "gft_build has not been called");
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

constexpr size_t kPinBuf = 128u << 20;       // bytes per bounce buffer
// what goes through a buffer at once (GFT_HOST_CHUNK_MB, 4 .. 128; timing study)
static size_t pin_chunk() {
    static const size_t n = [] {
        size_t mb = 128;
        if (const char* e = getenv("GFT_HOST_CHUNK_MB")) { const long v = atol(e); if (v >= 4 && v <= 128) mb = (size_t)v; }
        return mb << 20;
    }();
    return n;
}
#define kPinChunk pin_chunk()
// copy threads that fill a bounce buffer: the link (PCIe Gen5 x16, 57 GB/s from pinned memory) is only kept busy when the
// host side copies faster than that -- four threads reach ~58 GB/s, eight 120 (tools/probe_pcie.py); more than eight only add
// wake-ups (12: 11.4-12.0 M documents/s on the 250 000-document batch, 8: 12.2-12.3).  GFT_HOST_THREADS overrides
static unsigned pin_threads() {
    static const unsigned n = [] {
        if (const char* e = getenv("GFT_HOST_THREADS")) { const int v = atoi(e); if (v > 0) return (unsigned)std::min(v, 32); }
        const unsigned hc = std::thread::hardware_concurrency();
        return hc ? std::min(std::max(hc, 2u), 8u) : 4u;
    }();
    return n;
}

// the two pinned bounce buffers with their events, and the threads that fill / empty them
static int ensure_bounce(gft_engine* e) {
    for (int k = 0; k < 2; k++) {
        if (!e->pin[k]) HIP_TRY(hipHostMalloc(&e->pin[k], kPinBuf, hipHostMallocDefault), "pinned alloc");
        if (!e->pin_ev[k]) HIP_TRY(hipEventCreateWithFlags(&e->pin_ev[k], hipEventDisableTiming), "event");
    }
    if (!e->copy_pool) e->copy_pool.reset(new gft::CopyPool(pin_threads() - 1));
    return GFT_OK;
}

// pageable host memory -> device through the pinned bounce buffers
static int h2d_staged(gft_engine* e, void* dst, const void* src, size_t bytes) {
    if (bytes < (8u << 20)) {
        HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, e->stream), "upload");
        return GFT_OK;
    }
    if (int rc = ensure_bounce(e)) return rc;
    size_t done = 0;
    // (the first chunks are small and double: the link idles while the very first one is filled)
    size_t chunk = std::min<size_t>(kPinChunk, 4u << 20);
    for (int k = 0; done < bytes; k ^= 1, chunk = std::min(kPinChunk, chunk * 2)) {
        const size_t n = std::min(chunk, bytes - done);
        HIP_TRY(hipEventSynchronize(e->pin_ev[k]), "staging");        // the copy out of this buffer has finished
        e->copy_pool->copy(e->pin[k], (const uint8_t*)src + done, n);
        HIP_TRY(hipMemcpyAsync((uint8_t*)dst + done, e->pin[k], n, hipMemcpyHostToDevice, e->stream), "upload");
        HIP_TRY(hipEventRecord(e->pin_ev[k], e->stream), "staging");
        done += n;
    }
    return GFT_OK;
}

// device -> pageable host memory through the same bounce buffers (a copy straight into pageable memory is staged by the
// runtime through one thread); synchronous: returns when dst holds the bytes
static int d2h_staged(gft_engine* e, void* dst, const void* src, size_t bytes) {
    if (bytes < (8u << 20)) {
        HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, e->stream), "download");
        HIP_TRY(hipStreamSynchronize(e->stream), "download");
        return GFT_OK;
    }
    if (int rc = ensure_bounce(e)) return rc;
    size_t issued = 0, done = 0;
    size_t len[2] = {0, 0};
    int ki = 0, kd = 0;
    // chunk i + 1 is on the wire while chunk i is copied out of its buffer (a result smaller than two buffers goes in
    // quarters, so that there is a chunk i + 1)
    const size_t chunk = std::min(kPinChunk, std::max<size_t>(4u << 20, (bytes / 4 + 4095) & ~(size_t)4095));
    while (done < bytes) {
        while (issued < bytes && len[ki] == 0) {                  // (a buffer is free again once it has been copied out)
            const size_t n = std::min(chunk, bytes - issued);
            HIP_TRY(hipMemcpyAsync(e->pin[ki], (const uint8_t*)src + issued, n, hipMemcpyDeviceToHost, e->stream), "download");
            HIP_TRY(hipEventRecord(e->pin_ev[ki], e->stream), "staging");
            len[ki] = n; issued += n; ki ^= 1;
        }
        HIP_TRY(hipEventSynchronize(e->pin_ev[kd]), "staging");
        const size_t n = len[kd];
        e->copy_pool->copy((uint8_t*)dst + done, e->pin[kd], n);
        len[kd] = 0; done += n; kd ^= 1;
    }
    return GFT_OK;
}

static int stage_docs(gft_engine* e, const uint8_t* text_blob, const uint64_t* doc_off, uint64_t n_docs) {
    const uint64_t bytes = n_docs ? doc_off[n_docs] : 0;
    HIP_TRY(e->d_text.ensure(bytes + 64), "text alloc");
    HIP_TRY(e->d_doc_off.ensure((n_docs + 1) * 8), "doc_off alloc");
    if (bytes) { int rc = h2d_staged(e, e->d_text.p, text_blob, bytes); if (rc) return rc; }
    if (n_docs) HIP_TRY(hipMemcpyAsync(e->d_doc_off.p, doc_off, (n_docs + 1) * 8, hipMemcpyHostToDevice, e->stream), "doc_off upload");
    return GFT_OK;
}

int gft_scan(gft_engine* e, const uint8_t* text_blob, const uint64_t* doc_off, uint64_t n_docs, uint32_t flags,
             gft_matches* out) try {
    if (!e || !out || (n_docs && (!doc_off))) return e ? fail(e, GFT_E_INVALID, "null argument") : GFT_E_INVALID;
    GFT_LOCK(e);
    if (!e->peers.empty() && !e->in_multi && n_docs) return multi_scan(e, text_blob, doc_off, n_docs, flags, out);   // (an empty batch -- doc_off may be NULL -- is the first device's)
    if (e->device < 0) return fail(e, GFT_E_HIP, "no HIP device available");
    if (!e->built) return fail(e, GFT_E_NOT_BUILT, "gft_build has not been called");
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

int gft_set_programs(gft_engine* e, const uint32_t* prog_words, const uint64_t* prog_off, uint32_t n_exprs,
                     uint32_t n_extra) try {
    if (!e || (n_exprs && (!prog_words || !prog_off))) return e ? fail(e, GFT_E_INVALID, "null argument") : GFT_E_INVALID;
    GFT_LOCK(e);
    e->have_labels = false;     // (labels belong to a set of programs: gft_set_expr_labels)
    e->h_labels.clear();
    if (!e->peers.empty() && !e->in_multi) return multi_set_programs(e, prog_words, prog_off, n_exprs, n_extra);
    if (e->device < 0) return fail(e, GFT_E_HIP, "no HIP device available");
    if (!e->built) return fail(e, GFT_E_NOT_BUILT, "gft_build has not been called");
    ProgramSet ps;              // (declared before `drained`: the uploads below read it until the stream has drained)
    int rc = compile_programs(prog_words, prog_off, n_exprs, (uint32_t)e->tables.tab.terms.size() + n_extra, ps, e->err);
    if (rc) return rc;          // the handle is untouched: the set installed before, if any, still is
    refresh_options(e);
    if (e->opt_solve.dbg) print_program_stats(ps);
    DeviceGuard g(e->device);
    SyncOnExit drained(e);      // host buffers are read by asynchronous copies: drained on every way out
    // from here on the device holds a mixture of two sets until the last upload has landed: an error on the way leaves a
    // handle that answers GFT_E_NOT_BUILT, as after gft_build
    e->have_programs = false;
    e->n_exprs = 0;
    gft_engine::ProgramBufs& d = e->d_progs;
    if ((rc = upload(e, d.prog, ps.prog, "program upload"))) return rc;
    if ((rc = upload(e, d.prog_off, ps.prog_off, "program upload"))) return rc;
    if ((rc = upload(e, d.fprog, ps.fprog, "program upload"))) return rc;
    if ((rc = upload(e, d.fprog_off, ps.fprog_off, "program upload"))) return rc;
    if ((rc = upload(e, d.groups, ps.groups, "program upload"))) return rc;
    if ((rc = upload(e, d.order, ps.order, "program upload"))) return rc;
    if ((rc = upload(e, d.blk_class, ps.blk_class, "program upload"))) return rc;
    if ((rc = upload(e, d.wave_blk, ps.wave_blk, "program upload"))) return rc;
    if ((rc = upload(e, d.fprog_t, ps.fprog_t, "program upload"))) return rc;
    if ((rc = upload(e, d.fblk_off, ps.fblk_off, "program upload"))) return rc;
    if (ps.n_wide && (rc = upload(e, d.wide_list, ps.wide_list, "program upload"))) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream), "program upload");
    e->progs = std::move(ps);
    e->n_exprs = n_exprs; e->n_extra = n_extra; e->have_programs = true;
    e->pool.valid_docs = ~0ull;          // positions may not have been written for the old program set
    e->pool.csr_valid = false;
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
    if (e->device < 0) return fail(e, GFT_E_HIP, "no HIP device available");
    if (!e->built) return fail(e, GFT_E_NOT_BUILT, "gft_build has not been called");
    if (!e->have_programs) return fail(e, GFT_E_NOT_BUILT, "gft_set_programs has not been called");
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
    if (!pend_settled(e)) return fail(e, GFT_E_INVALID, "batches of gft_process_device_begin are in flight: gft_process_device_end (or _complete) first");
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
    if (e->device < 0) return fail(e, GFT_E_HIP, "no HIP device available");
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
        HIP_TRY(e->d_cp_cnt.ensure(n_docs * 4), "compact alloc");
        HIP_TRY(e->d_cp_partial.ensure(scan_partials_needed(n_docs) * 8), "compact alloc");
        {
            ProfScope ps(e, "compact_count");
            HIP_TRY(launch_compact_count(d_bitmap, n_docs, e->n_exprs, e->d_cp_cnt.as<uint32_t>(), e->n_cus, st), "compact count");
        }
        {
            ProfScope ps(e, "compact_scan");
            HIP_TRY(launch_exclusive_scan(e->d_cp_cnt.as<uint32_t>(), n_docs, d_row_off, e->d_cp_partial.as<uint64_t>(), st), "compact scan");
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
    e->h_row_off.assign(n_docs + 1, 0);
    const uint32_t* labels = e->have_labels ? e->h_labels.data() : nullptr;
    const uint64_t total = compact_host(h_bitmap, n_docs, e->n_exprs, labels, e->h_row_off.data(), nullptr, nullptr, 0);
    e->h_expr_idx.assign(total + 1, 0);
    e->h_label.assign(labels ? total + 1 : 1, 0);
    compact_host(h_bitmap, n_docs, e->n_exprs, labels, e->h_row_off.data(), e->h_expr_idx.data(), labels ? e->h_label.data() : nullptr, total);
    out->n_docs = n_docs; out->total = total;
    out->row_off = e->h_row_off.data(); out->expr_idx = e->h_expr_idx.data(); out->label = labels ? e->h_label.data() : nullptr;
}

// ... of a bitmap that is complete on the DEVICE: compacted there, only the CSR comes down (staged like every large result)
int sparse_from_device(gft_engine* e, const uint32_t* d_bitmap, uint64_t n_docs, gft_sparse* out) {
    HIP_TRY(e->d_cp_row_off.ensure((n_docs + 1) * 8), "compact alloc");
    int rc = compact_enqueue(e, d_bitmap, n_docs, e->d_cp_row_off.as<uint64_t>(), nullptr, nullptr, 0, true, false);
    if (rc) return rc;
    e->h_row_off.assign(n_docs + 1, 0);
    if ((rc = d2h_staged(e, e->h_row_off.data(), e->d_cp_row_off.p, (n_docs + 1) * 8))) return rc;
    const uint64_t total = e->h_row_off[n_docs];
    const bool labels = e->have_labels;
    e->h_expr_idx.assign(total + 1, 0);
    e->h_label.assign(labels ? total + 1 : 1, 0);
    if (total) {
        HIP_TRY(e->d_cp_idx.ensure(total * 4), "compact alloc");
        if (labels) HIP_TRY(e->d_cp_label.ensure(total * 4), "compact alloc");
        rc = compact_enqueue(e, d_bitmap, n_docs, e->d_cp_row_off.as<uint64_t>(), e->d_cp_idx.as<uint32_t>(),
                             labels ? e->d_cp_label.as<uint32_t>() : nullptr, total, false, true);
        if (rc) return rc;
        if ((rc = d2h_staged(e, e->h_expr_idx.data(), e->d_cp_idx.p, total * 4))) return rc;
        if (labels && (rc = d2h_staged(e, e->h_label.data(), e->d_cp_label.p, total * 4))) return rc;
    }
    out->n_docs = n_docs; out->total = total;
    out->row_off = e->h_row_off.data(); out->expr_idx = e->h_expr_idx.data(); out->label = labels ? e->h_label.data() : nullptr;
    return GFT_OK;
}

int process_host(gft_engine* e, const uint8_t* text_blob, const uint64_t* doc_off, uint64_t n_docs, uint32_t flags,
                 const gft_extra_matches* extra, uint32_t* hit_bitmap, gft_sparse* sparse);

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
        e->h_sparse_bm.assign(n_docs * ((e->n_exprs + 31) / 32) + 1, 0);
        const int rc = multi_process(e, text_blob, doc_off, n_docs, flags, extra, e->h_sparse_bm.data());
        if (rc) return rc;
        sparse_from_host(e, e->h_sparse_bm.data(), n_docs, out);
        return GFT_OK;
    }
    return process_host(e, text_blob, doc_off, n_docs, flags, extra, nullptr, out);
} GFT_CATCH((e ? &e->err : nullptr))

namespace {

// gft_process, and gft_process_sparse (sparse != nullptr: the CSR instead of the rows) on one device
int process_host(gft_engine* e, const uint8_t* text_blob, const uint64_t* doc_off, uint64_t n_docs, uint32_t flags,
                 const gft_extra_matches* extra, uint32_t* hit_bitmap, gft_sparse* sparse) {
    if (e->device < 0) return fail(e, GFT_E_HIP, "no HIP device available");
    if (!e->built) return fail(e, GFT_E_NOT_BUILT, "gft_build has not been called");
    if (!e->have_programs) return fail(e, GFT_E_NOT_BUILT, "gft_set_programs has not been called");
    if (!pend_settled(e)) return fail(e, GFT_E_INVALID, "batches of gft_process_device_begin are in flight: gft_process_device_end (or _complete) first");
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
        e->h_sparse_bm.assign(n_docs * words + 1, 0);
        hit_bitmap = e->h_sparse_bm.data();
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

int gft_set_expr_labels(gft_engine* e, const uint32_t* labels, uint32_t n) try {
    if (!e) return GFT_E_INVALID;
    GFT_LOCK(e);
    e->have_labels = false;
    e->h_labels.clear();
    if (!labels || !n) {
        if (labels || n) return fail(e, GFT_E_INVALID, "gft_set_expr_labels: labels and n go together (NULL, 0 clears)");
        return GFT_OK;
    }
    if (!e->have_programs) return fail(e, GFT_E_NOT_BUILT, "gft_set_programs has not been called");
    if (n != e->n_exprs) return fail(e, GFT_E_INVALID, "gft_set_expr_labels: one label per expression (n != gft_n_exprs)");
    if (e->device < 0) return fail(e, GFT_E_HIP, "no HIP device available");
    DeviceGuard g(e->device);
    SyncOnExit drained(e);
    e->h_labels.assign(labels, labels + n);
    const int rc = upload(e, e->d_labels, e->h_labels, "label upload");
    if (rc) { e->h_labels.clear(); return rc; }
    e->have_labels = true;
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

int gft_compact_device(gft_engine* e, const uint32_t* d_hit_bitmap, uint64_t n_docs, uint64_t* d_row_off, uint32_t* d_expr_idx,
                       uint32_t* d_label, uint64_t cap, uint64_t* total) try {
    if (!e || !d_row_off) return e ? fail(e, GFT_E_INVALID, "null argument") : GFT_E_INVALID;
    GFT_LOCK(e);
    if (!e->peers.empty()) return fail(e, GFT_E_UNSUPPORTED, "gft_compact_device: single-device handles only (sparse gathers between devices are not built)");
    if (e->device < 0) return fail(e, GFT_E_HIP, "no HIP device available");
    if (!e->have_programs) return fail(e, GFT_E_NOT_BUILT, "gft_set_programs has not been called");
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


namespace {

// strings.ToLower of a batch, first half: the unit table, the count pass, the prefix sum and d_out_off (complete when this
// returns GFT_OK; the stream has drained).  *n_units / *total: what lower_write needs and what the caller sizes its buffer by.
// d_out / cap take part in the overlap check only.
int lower_count(gft_engine* e, const uint8_t* d_text, const uint64_t* d_doc_off, uint64_t n_docs, const uint8_t* d_out, uint64_t cap,
                uint64_t* d_out_off, uint64_t* n_units, uint64_t* total) {
    hipStream_t st = e->stream;
    *n_units = 0; *total = 0;
    if (!n_docs) {
        HIP_TRY(hipMemsetAsync(d_out_off, 0, 8, st), "lower offsets");
        HIP_TRY(hipStreamSynchronize(st), "lower offsets");
        return GFT_OK;
    }
    if (!e->lower_table_up) {
        const LowerTableHost& t = lower_table_host();
        int rc = upload(e, e->d_lw_page, t.page, "lower table upload");
        if (!rc) rc = upload(e, e->d_lw_delta, t.delta, "lower table upload");
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(st), "lower table upload");
        e->lower_table_up = true;
    }
    const LowerTable T{e->d_lw_page.as<uint16_t>(), e->d_lw_delta.as<int32_t>(), (uint32_t)lower_table_host().page.size()};
    // d_lw_ctl: [0] units, [1] first and [2] last text offset (k_pack_ctl), [3] flags: 1 a document of 4 GiB or more or
    // descending offsets (k_unit_count), 2 a lowered document of 4 GiB or more (k_lower_offsets)
    HIP_TRY(e->d_lw_ctl.ensure(32), "lower alloc");
    HIP_TRY(e->d_lw_doc_units.ensure(n_docs * 4), "lower alloc");
    HIP_TRY(e->d_lw_unit_base.ensure((n_docs + 1) * 8), "lower alloc");
    HIP_TRY(e->d_lw_partial.ensure(scan_partials_needed(n_docs) * 8), "lower alloc");
    uint64_t* ctl = e->d_lw_ctl.as<uint64_t>();
    uint32_t* flags = reinterpret_cast<uint32_t*>(ctl + 3);
    uint64_t h_ctl[4] = {0, 0, 0, 0};
    {
        ProfScope ps(e, "aux");
        HIP_TRY(hipMemsetAsync(ctl, 0, 32, st), "lower units");
        HIP_TRY(launch_unit_count(d_doc_off, n_docs, kLowerUnitMax, e->d_lw_doc_units.as<uint32_t>(), flags, st), "lower units");
        HIP_TRY(launch_exclusive_scan(e->d_lw_doc_units.as<uint32_t>(), n_docs, e->d_lw_unit_base.as<uint64_t>(), e->d_lw_partial.as<uint64_t>(), st),
                "lower units");
        HIP_TRY(launch_pack_ctl(e->d_lw_unit_base.as<uint64_t>(), d_doc_off, n_docs, ctl, st), "lower units");
    }
    HIP_TRY(hipMemcpyAsync(h_ctl, ctl, 32, hipMemcpyDeviceToHost, st), "lower units");
    HIP_TRY(hipStreamSynchronize(st), "lower units");
    if (h_ctl[3] & 1) return fail(e, GFT_E_INVALID, "gft_to_lower_device: document offsets descend, or a document of 4 GiB or more");
    if (lower_buffers_overlap(d_text, h_ctl[1], h_ctl[2], d_doc_off, n_docs, d_out, cap, d_out_off))
        return fail(e, GFT_E_INVALID, "gft_to_lower_device: the output overlaps the input");
    const uint64_t nu = h_ctl[0];
    HIP_TRY(e->d_lw_units.ensure(nu * sizeof(Unit)), "lower alloc");
    HIP_TRY(e->d_lw_unit_cnt.ensure(nu * 4), "lower alloc");
    HIP_TRY(e->d_lw_unit_out.ensure((nu + 1) * 8), "lower alloc");
    HIP_TRY(e->d_lw_partial.ensure(scan_partials_needed(nu) * 8), "lower alloc");
    {
        ProfScope ps(e, "aux");
        HIP_TRY(launch_unit_fill(d_doc_off, n_docs, e->d_lw_unit_base.as<uint64_t>(), e->d_lw_units.as<Unit>(), kLowerUnitMax, st, nu), "lower units");
    }
    {
        ProfScope ps(e, "lower_count");
        HIP_TRY(launch_lower_count(d_text, d_doc_off, e->d_lw_units.as<Unit>(), nu, T, e->d_lw_unit_cnt.as<uint32_t>(), e->n_cus, st), "lower count");
    }
    {
        ProfScope ps(e, "lower_scan");
        HIP_TRY(launch_exclusive_scan(e->d_lw_unit_cnt.as<uint32_t>(), nu, e->d_lw_unit_out.as<uint64_t>(), e->d_lw_partial.as<uint64_t>(), st), "lower scan");
        HIP_TRY(launch_lower_offsets(e->d_lw_unit_base.as<uint64_t>(), e->d_lw_unit_out.as<uint64_t>(), n_docs, d_out_off, flags, st), "lower scan");
    }
    HIP_TRY(hipMemcpyAsync(h_ctl, e->d_lw_unit_out.as<uint64_t>() + nu, 8, hipMemcpyDeviceToHost, st), "lower total");
    HIP_TRY(hipMemcpyAsync(h_ctl + 3, ctl + 3, 8, hipMemcpyDeviceToHost, st), "lower total");
    HIP_TRY(hipStreamSynchronize(st), "lower count");
    if (h_ctl[3] & 2) return fail(e, GFT_E_INVALID, "gft_to_lower_device: the lower-case form of a document has 4 GiB or more");
    *n_units = nu; *total = h_ctl[0];
    return GFT_OK;
}

// ... second half: the write pass over the unit table and prefix sums lower_count left in the engine.  Nothing waits here.
int lower_write(gft_engine* e, const uint8_t* d_text, const uint64_t* d_doc_off, uint64_t n_units, uint8_t* d_out, uint64_t cap) {
    if (!n_units || !cap) return GFT_OK;
    const LowerTable T{e->d_lw_page.as<uint16_t>(), e->d_lw_delta.as<int32_t>(), (uint32_t)lower_table_host().page.size()};
    ProfScope ps(e, "lower_write");
    HIP_TRY(launch_lower_write(d_text, d_doc_off, e->d_lw_units.as<Unit>(), n_units, T, e->d_lw_unit_out.as<uint64_t>(), d_out, cap, e->n_cus,
                               e->stream), "lower write");
    return GFT_OK;
}

int lower_entry_checks(gft_engine* e, const char* who) {
    if (!e->peers.empty()) return fail(e, GFT_E_UNSUPPORTED, std::string(who) + ": single-device handles only");
    if (e->device < 0) return fail(e, GFT_E_HIP, "no HIP device available");
    if (!pend_settled(e))
        return fail(e, GFT_E_INVALID, std::string(who) + ": batches of gft_process_device_begin are in flight: gft_process_device_end (or _complete) first");
    return GFT_OK;
}

}  // namespace

int gft_to_lower_device(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint8_t* d_out, uint64_t cap,
                        uint64_t* d_out_off, uint64_t* total) try {
    if (!e || !d_out_off || (n_docs && !d_doc_off)) return e ? fail(e, GFT_E_INVALID, "null argument") : GFT_E_INVALID;
    GFT_LOCK(e);
    if (cap && !d_out) return fail(e, GFT_E_INVALID, "gft_to_lower_device: cap bytes but no output buffer");
    int rc = lower_entry_checks(e, "gft_to_lower_device");
    if (rc) return rc;
    DeviceGuard g(e->device);
    uint64_t n_units = 0, n_total = 0;
    if ((rc = lower_count(e, d_text_blob, d_doc_off, n_docs, d_out, cap, d_out_off, &n_units, &n_total))) return rc;
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
    if ((rc = room(e->d_lw_off, (n_docs + 1) * 8))) return rc;
    uint64_t n_units = 0, total = 0;
    if ((rc = lower_count(e, d_text_blob, d_doc_off, n_docs, nullptr, 0, e->d_lw_off.as<uint64_t>(), &n_units, &total))) return rc;
    if ((rc = room(e->d_lw_text, total + 64))) return rc;
    if ((rc = lower_write(e, d_text_blob, d_doc_off, n_units, e->d_lw_text.as<uint8_t>(), total))) return rc;
    *d_lowered = e->d_lw_text.as<uint8_t>();
    *d_lowered_off = e->d_lw_off.as<uint64_t>();
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

// ---- rule evaluation for records (gft_rules.hpp) ---------------------------------------------------------------------
}  // extern "C"

namespace {
int rules_entry_checks(gft_engine* e) {
    if (!e->peers.empty()) return fail(e, GFT_E_UNSUPPORTED, "record batches: single-device handles only");
    if (e->device < 0) return fail(e, GFT_E_HIP, "no HIP device available");
    if (!pend_settled(e))
        return fail(e, GFT_E_INVALID, "record batches: batches of gft_process_device_begin are in flight: gft_process_device_end (or _complete) first");
    return GFT_OK;
}
int rules_room(gft_engine* e, DevBuf& b, uint64_t bytes) {
    const hipError_t h = b.ensure(std::max<uint64_t>(bytes, 16));
    if (h == hipErrorOutOfMemory) { (void)hipGetLastError(); return fail(e, GFT_E_NOMEM, "no device memory for the record batch's work buffers"); }
    return h == hipSuccess ? (int)GFT_OK : fail_hip(e, h, "record batch alloc");
}
}  // namespace

namespace gft {

void rules_lock(gft_engine* e) { e->mu.lock(); }
void rules_unlock(gft_engine* e) { e->mu.unlock(); }

int rules_install(gft_engine* e, const RuleSet& rs, uint64_t* serial) try {
    if (!e || !serial) return GFT_E_INVALID;
    GFT_LOCK(e);
    int rc = rules_entry_checks(e);
    if (rc) return rc;
    if (rules_lds_bytes(rs.n_units(), rs.max_depth) + 64 > e->lds_max)
        return fail(e, GFT_E_UNSUPPORTED, "record rules: the UNIT words and operand stacks of this set do not fit the device's LDS");
    DeviceGuard g(e->device);
    auto& R = e->d_rules;
    R.serial = 0;                          // (a failed upload leaves no set)
    if ((rc = upload(e, R.expr_tag, rs.expr_tag, "rule set upload"))) return rc;
    if ((rc = upload(e, R.masks, rs.masks, "rule set upload"))) return rc;
    if ((rc = upload(e, R.units, rs.units, "rule set upload"))) return rc;
    if ((rc = upload(e, R.prog, rs.prog, "rule set upload"))) return rc;
    if ((rc = upload(e, R.prog_off, rs.prog_off, "rule set upload"))) return rc;
    HIP_TRY(R.flags.ensure(16), "rule set upload");
    HIP_TRY(hipStreamSynchronize(e->stream), "rule set upload");
    R.n_fields = rs.n_fields; R.n_tags = rs.n_tags; R.n_exprs = rs.n_exprs; R.n_rules = rs.n_rules;
    R.n_units = rs.n_units(); R.max_depth = rs.max_depth; R.field_words = rs.field_words;
    static std::atomic<uint64_t> next_serial{1};
    *serial = R.serial = next_serial.fetch_add(1);
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

uint64_t rules_serial(gft_engine* e) {
    if (!e) return 0;
    GFT_LOCK(e);
    return e->d_rules.serial;
}

int rules_leaf_bitmap(gft_engine* e, uint64_t n_leaves, uint32_t words, uint32_t** d_bitmap) try {
    if (!e || !d_bitmap) return GFT_E_INVALID;
    GFT_LOCK(e);
    int rc = rules_entry_checks(e);
    if (rc) return rc;
    DeviceGuard g(e->device);
    if ((rc = rules_room(e, e->d_rules.leaf_bitmap, n_leaves * words * 4))) return rc;
    *d_bitmap = e->d_rules.leaf_bitmap.as<uint32_t>();
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

int rules_stage(gft_engine* e, int n, const void* const* src, const uint64_t* bytes, const uint64_t* slack, void** d_dst) try {
    if (!e || n < 0 || n > 6 || (n && (!src || !bytes || !slack || !d_dst))) return GFT_E_INVALID;
    GFT_LOCK(e);
    int rc = rules_entry_checks(e);
    if (rc) return rc;
    DeviceGuard g(e->device);
    SyncOnExit drain(e);
    for (int k = 0; k < n; k++) {
        DevBuf& b = e->d_rules.stage[k];
        if ((rc = rules_room(e, b, bytes[k] + slack[k]))) return rc;
        if (bytes[k]) HIP_TRY(hipMemcpyAsync(b.p, src[k], bytes[k], hipMemcpyHostToDevice, e->stream), "record batch upload");
        if (slack[k]) HIP_TRY(hipMemsetAsync((uint8_t*)b.p + bytes[k], 0, slack[k], e->stream), "record batch upload");
        d_dst[k] = b.p;
    }
    HIP_TRY(hipStreamSynchronize(e->stream), "record batch upload");
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

int rules_fetch(gft_engine* e, void* dst, const void* d_src, uint64_t bytes) try {
    if (!e || (bytes && (!dst || !d_src))) return GFT_E_INVALID;
    GFT_LOCK(e);
    DeviceGuard g(e->device);
    SyncOnExit drain(e);
    if (bytes) HIP_TRY(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, e->stream), "rule bitmap download");
    HIP_TRY(hipStreamSynchronize(e->stream), "rule bitmap download");
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

int rules_eval_device(gft_engine* e, const uint32_t* d_hit_bitmap, const uint32_t* d_leaf_field, const uint64_t* d_rec_off,
                          uint64_t n_records, uint64_t n_leaves, uint32_t* d_rule_bitmap) try {
    if (!e) return GFT_E_INVALID;
    GFT_LOCK(e);
    int rc = rules_entry_checks(e);
    if (rc) return rc;
    auto& R = e->d_rules;
    if (!R.serial) return fail(e, GFT_E_INVALID, "record rules: no rule set installed");
    // (what validate_records refuses on the host is refused here: the kernels check fields and offsets also when no rule reads them)
    if (!n_records) return n_leaves ? fail(e, GFT_E_INVALID, "record batch: leaves but no records") : (int)GFT_OK;
    if (!d_rec_off || (R.n_rules && !d_rule_bitmap) || (n_leaves && (!d_leaf_field || (R.n_exprs && !d_hit_bitmap))))
        return fail(e, GFT_E_INVALID, "record batch: null argument");
    DeviceGuard g(e->device);
    hipStream_t st = e->stream;
    const uint32_t TW = (R.n_tags + 31) / 32;
    if ((rc = rules_room(e, R.tag_rows, n_leaves * TW * 4))) return rc;
    uint32_t* d_flags = R.flags.as<uint32_t>();
    HIP_TRY(hipMemsetAsync(d_flags, 0, 8, st), "record rules");
    {
        ProfScope ps(e, "group_tags");
        HIP_TRY(launch_leaf_tags(d_hit_bitmap, R.n_exprs, R.expr_tag.as<uint32_t>(), d_leaf_field, R.n_fields, n_leaves, R.n_tags,
                                 R.tag_rows.as<uint32_t>(), d_flags, st), "leaf tag kernel launch");
    }
    RulesParams P{};
    P.tag_rows = R.tag_rows.as<uint32_t>();
    P.leaf_field = d_leaf_field;
    P.rec_off = d_rec_off;
    P.n_records = n_records; P.n_leaves = n_leaves;
    P.masks = R.masks.as<uint32_t>(); P.units = R.units.as<uint32_t>();
    P.prog = R.prog.as<uint32_t>(); P.prog_off = R.prog_off.as<uint32_t>();
    P.TW = TW; P.FW = R.field_words; P.RW = (R.n_rules + 31) / 32;
    P.n_fields = R.n_fields; P.n_units = R.n_units; P.n_rules = R.n_rules; P.max_depth = R.max_depth;
    P.flags = d_flags; P.out = d_rule_bitmap;
    {
        ProfScope ps(e, "group_rules");
        HIP_TRY(launch_record_rules(P, e->lds_max, st), "record rule kernel launch");
    }
    uint32_t h_flags[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(h_flags, d_flags, 8, hipMemcpyDeviceToHost, st), "record rules");
    HIP_TRY(hipStreamSynchronize(st), "record rules");
    if (h_flags[1]) return fail(e, GFT_E_INVALID, "record batch: rec_off descends or does not end at n_leaves");
    if (h_flags[0]) return fail(e, GFT_E_INVALID, "record batch: a leaf names a field outside the schema");
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

}  // namespace gft

extern "C" {

int gft_debug_emulate_scan(const uint8_t* terms_blob, const uint64_t* term_off, uint32_t n_terms, const uint8_t* text,
                           uint32_t len, uint32_t lo, uint32_t flags, uint32_t scan_flags, uint32_t* out_term,
                           uint32_t* out_pos, uint64_t cap, uint64_t* needed) try {
    if ((n_terms && (!terms_blob || !term_off)) || (len && !text) || lo > len || !needed) return GFT_E_INVALID;
    std::vector<std::string> terms;
    for (uint32_t i = 0; i < n_terms; i++) terms.emplace_back((const char*)terms_blob + term_off[i], (size_t)(term_off[i + 1] - term_off[i]));
    AcTables tab;
    build_ac_tables(std::move(terms), tab);
    Scan3Tables t;
    build_scan3_tables(tab, t);
    if (!t.supported) return GFT_E_UNSUPPORTED;
    std::vector<Scan3Hit> hits;
    scan3_emulate(t, text, len, lo, (scan_flags & GFT_FOLD_ASCII) != 0, (flags & GFT_POS_END) != 0, hits);
    *needed = hits.size();
    if (hits.size() > cap || (hits.size() && (!out_term || !out_pos))) return GFT_E_INVALID;
    for (size_t i = 0; i < hits.size(); i++) { out_term[i] = hits[i].term; out_pos[i] = hits[i].pos; }
    return GFT_OK;
} GFT_CATCH(nullptr)

int gft_debug_scan5_filter(const uint8_t* terms_blob, const uint64_t* term_off, uint32_t n_terms, const uint8_t* text, uint32_t len,
                           uint32_t lane_start, uint32_t scan_flags, uint32_t groups, uint8_t* out_exact, uint8_t* out_dual,
                           uint32_t* groups_used) try {
    if ((n_terms && (!terms_blob || !term_off)) || (len && (!text || !out_exact || !out_dual)) || lane_start > len) return GFT_E_INVALID;
    std::vector<std::string> terms;
    for (uint32_t i = 0; i < n_terms; i++) terms.emplace_back((const char*)terms_blob + term_off[i], (size_t)(term_off[i + 1] - term_off[i]));
    AcTables tab;
    build_ac_tables(std::move(terms), tab);
    Scan2Tables s2;
    build_scan2_tables(tab, s2);
    if (!s2.long_ok) return GFT_E_UNSUPPORTED;
    Scan5Tables s5;
    // (a filter word has one bit per group: 32 at most, whatever the caller asks for; the kernel's plan stops at kScan5MaxGroups)
    build_scan5_tables(tab, s2, std::min<uint32_t>(groups && groups < s2.kp ? groups : s2.kp, 32u), s5);
    if (groups_used) *groups_used = s5.G;
    const bool fold = (scan_flags & GFT_FOLD_ASCII) != 0;
    const uint8_t* cls = fold ? s2.cls_fold : s2.cls;
    const uint8_t* grp = fold ? s5.grp_fold : s5.grp;
    const uint32_t kp = s2.kp, G = s5.G;
    // the exact filter, from first principles (whatever the alphabet): the 4-window of exact classes that ends at i is the
    // anchor window of a long term (= a key of the bucket table), or a term of length <= 3 ends at i; the pad class stands in
    // front of the document
    auto cl = [&](int64_t i) { return i < 0 ? s2.pad_class : (uint32_t)cls[text[i]]; };
    auto gr = [&](int64_t i) { return i < 0 ? s5.pad_group : (uint32_t)grp[text[i]]; };
    std::unordered_set<uint32_t> keys;
    for (const Scan2Slot& sl : s2.slots) if (sl.key != kScan2EmptyKey) keys.insert(sl.key);
    std::vector<std::vector<uint32_t>> shorts;
    for (const auto& term : tab.terms)
        if (!term.empty() && term.size() < 4) {
            std::vector<uint32_t> v;
            for (unsigned char ch : term) v.push_back(tab.byte_class[ch]);
            shorts.push_back(v);
        }
    for (uint32_t i = 0; i < len; i++) {
        const uint32_t key = (uint32_t)((((uint64_t)cl((int64_t)i - 3) * kp + cl((int64_t)i - 2)) * kp + cl((int64_t)i - 1)) * kp + cl(i));
        bool f = keys.count(key) != 0;
        for (size_t k = 0; k < shorts.size() && !f; k++) {
            const auto& v = shorts[k];
            bool eq = true;
            for (size_t j = 0; j < v.size() && eq; j++) eq = cl((int64_t)i - (int64_t)(v.size() - 1 - j)) == v[j];
            f = eq;
        }
        out_exact[i] = f ? 1 : 0;
        out_dual[i] = 0;
    }
    // gft_scan5.hip: probes at lane_start, lane_start + 2, ...; the probe at j reads entry (g[j-2], g[j-1], g[j]): bit g[j-3] of
    // its low word is the flag of j, bit g[j+1] of its high word the flag of j + 1.  (Positions in front of lane_start belong
    // to the lane before: walked here with the same parity, so that every position is answered once.)
    for (int64_t j = (int64_t)(lane_start & 1u); j < (int64_t)len; j += 2) {
        const uint64_t ent = s5.filter[((size_t)gr(j - 2) * G + gr(j - 1)) * G + gr(j)];
        out_dual[j] = (uint8_t)(ent >> gr(j - 3) & 1);
        if (j + 1 < (int64_t)len) out_dual[j + 1] = (uint8_t)(ent >> (32 + gr(j + 1)) & 1);
    }
    if (lane_start & 1u) {                                   // position 0 is the second half of a probe at -1
        const uint64_t ent = s5.filter[((size_t)gr(-3) * G + gr(-2)) * G + gr(-1)];
        if (len) out_dual[0] = (uint8_t)(ent >> (32 + gr(0)) & 1);
    }
    return GFT_OK;
} GFT_CATCH(nullptr)

int gft_debug_program_shape(const uint32_t* prog_words, const uint64_t* prog_off, uint32_t n_exprs, uint32_t n_slots, uint32_t* out_shape,
                            uint32_t shape_cap) try {
    if (!prog_words || !prog_off || !out_shape || n_slots > (1u << kDwFieldBits)) return GFT_E_INVALID;
    ProgramSet ps;
    std::string err;
    const int rc = compile_programs(prog_words, prog_off, n_exprs, n_slots, ps, err);
    if (rc) return rc;
    if (shape_cap < 3 + ps.blk_class.size()) return GFT_E_INVALID;
    out_shape[0] = ps.fprog_words; out_shape[1] = ps.n_rare_words > 0; out_shape[2] = ps.wide_pairs;
    std::copy(ps.blk_class.begin(), ps.blk_class.end(), out_shape + 3);
    return GFT_OK;
} GFT_CATCH(nullptr)

int gft_debug_eval_programs(const uint32_t* prog_words, const uint64_t* prog_off, uint32_t n_exprs, uint32_t n_slots,
                            const uint8_t* present, uint8_t* out_hit, uint32_t* out_depth) try {
    if (!prog_words || !prog_off || !out_hit || (n_slots && !present) || n_slots > (1u << kDwFieldBits)) return GFT_E_INVALID;
    ProgramSet ps;
    std::string err;
    const int rc = compile_programs(prog_words, prog_off, n_exprs, n_slots, ps, err);
    if (rc) return rc;
    std::vector<uint8_t> elsewhere(n_exprs, 0);      // answered by the host, or by the solver's second phase: a stand-in here
    for (uint32_t x : ps.host_only) elsewhere[x] = 1;
    for (uint32_t k = 0; k < ps.n_wide; k++) elsewhere[ps.wide_list[3 * k]] = 1;
    for (uint32_t i = 0; i < n_exprs; i++) {
        // expression ex the way its lane reads it (gft_solve.hip run_program_far): sorted position i = lane i % 64 of block i / 64
        const uint32_t ex = ps.order[i], b = i / 64, lane = i % 64;
        if (elsewhere[ex]) return GFT_E_UNSUPPORTED;
        const uint32_t depth = ps.fdepth[ex];
        if (out_depth) out_depth[ex] = depth;
        // the device's data flow on one document (gft_kernels.hpp "What the kernel reads", gft_solve.hip run_program)
        bool acc = false;
        std::vector<bool> stack;
        size_t reached = 0;
        for (uint64_t pc = 0; pc < ps.fprog_off[ex + 1] - ps.fprog_off[ex]; pc++) {
            const uint32_t w = ps.fprog_t[ps.fblk_off[b] + ((pc / 4) * 64 + lane) * 4 + pc % 4];
            if (w & kDwRare) {
                if (!(w & kDwNeg)) return GFT_E_UNSUPPORTED;         // an INORD group: needs positions
                acc = !acc;
                continue;
            }
            const bool v = (present[(w & kDwFieldMask) >> kDwFieldShift] != 0) != ((w & kDwNeg) != 0);
            if ((w & kDwPop) && stack.empty()) return GFT_E_INVALID;
            const bool x = (w & kDwPop) ? (bool)stack.back() : v;
            const bool A = (w & kDwSel) ? x : (w & kDwOnes) != 0, B = (w & kDwOr) ? x : false;
            const bool before = acc;
            acc = (acc && A) || B;
            if (w & kDwPop) stack.pop_back();
            if (w & kDwPush) stack.push_back(before);
            if (stack.size() > depth) return GFT_E_INVALID;           // fuse_program's own depth figure must hold
            reached = std::max(reached, stack.size());
        }
        if (!stack.empty()) return GFT_E_INVALID;
        // ... and fits the interpreter its block was given
        if (reached > (ps.blk_class[b] == 0 ? 0u : ps.blk_class[b] == 1 ? kSolveRegStack : kMaxBoolDepth)) return GFT_E_INTERNAL;
        out_hit[ex] = acc ? 1 : 0;
    }
    return GFT_OK;
} GFT_CATCH(nullptr)

// what gft_debug_tables and gft_debug_scan_plan share: the table set (compiled from the terms, or read from `blob`) and the plan
// that plan_scan makes for it
static int debug_tables_and_plan(const uint8_t* terms_blob, const uint64_t* term_off, uint32_t n_terms, const uint8_t* blob, uint64_t blob_len,
                                 uint64_t lds_max, const char* forced_kernel, TableSet& set, uint32_t& flags, ScanPlan& plan, std::string& err) {
    if (blob) {
        if (int rc = read_tables(blob, blob_len, set, flags, err)) return rc;
    } else {
        std::vector<std::string> terms;
        for (uint32_t i = 0; i < n_terms; i++) terms.emplace_back((const char*)terms_blob + term_off[i], (size_t)(term_off[i + 1] - term_off[i]));
        compile_tables(std::move(terms), set);
    }
    ScanOptions opt = scan_options();
    if (forced_kernel) opt.forced = parse_forced(forced_kernel);
    return plan_scan(set, opt, lds_max, kExtraKernels, plan, err);
}

int gft_debug_tables(const uint8_t* terms_blob, const uint64_t* term_off, uint32_t n_terms, const uint8_t* blob, uint64_t blob_len,
                     uint64_t lds_max, const char* forced_kernel, const char** kernel, uint8_t* out, uint64_t cap, uint64_t* needed,
                     char* err_out, uint64_t err_cap) try {
    if (!kernel || !needed || (!blob && n_terms && (!terms_blob || !term_off))) return GFT_E_INVALID;
    *kernel = "";
    *needed = 0;
    std::string err;
    auto done = [&](int rc) {
        if (err_out && err_cap) { const size_t n = std::min<size_t>(err.size(), err_cap - 1); memcpy(err_out, err.data(), n); err_out[n] = 0; }
        return rc;
    };
    TableSet set;
    uint32_t flags = 0;
    int rc;
    ScanPlan plan;
    if ((rc = debug_tables_and_plan(terms_blob, term_off, n_terms, blob, blob_len, lds_max, forced_kernel, set, flags, plan, err))) return done(rc);
    *kernel = kScanKernelName[(int)plan.kernel];
    if (plan.kernel == ScanKernel::scan5) {              // (what gft_build would go on to derive: it must not fault on these tables)
        Scan5Tables s5;
        std::vector<uint32_t> bloom;
        derive_scan5(set, plan, s5, bloom);
    }
    std::vector<uint8_t> b;
    write_tables(set, flags, b);
    *needed = b.size();
    if (!out) return done(GFT_OK);
    if (cap < b.size()) return done(GFT_E_INVALID);
    memcpy(out, b.data(), b.size());
    return done(GFT_OK);
} GFT_CATCH(nullptr)

int gft_debug_learned_unit(const gft_engine* e, uint32_t* unit_max, uint32_t* fifo_cap) {
    if (!e || !unit_max) return GFT_E_INVALID;
    *unit_max = e->learned.unit_max;
    if (fifo_cap) *fifo_cap = e->plan.kernel == ScanKernel::scan5 ? e->plan.s5plan.fifo_cap : kScan2FifoCap;
    return GFT_OK;
}

int gft_debug_scan_plan(const uint8_t* terms_blob, const uint64_t* term_off, uint32_t n_terms, uint64_t lds_max, const char* forced_kernel,
                        const char** kernel, uint32_t* plan_out) try {
    if (!kernel || !plan_out || (n_terms && (!terms_blob || !term_off))) return GFT_E_INVALID;
    *kernel = "";
    TableSet set;
    uint32_t flags = 0;
    ScanPlan plan;
    std::string err;
    if (int rc = debug_tables_and_plan(terms_blob, term_off, n_terms, nullptr, 0, lds_max, forced_kernel, set, flags, plan, err)) return rc;
    *kernel = kScanKernelName[(int)plan.kernel];
    const bool s5 = plan.kernel == ScanKernel::scan5;
    plan_out[0] = set.tab.max_term_len;
    plan_out[1] = s5 ? plan.s5_term_bits : 0u;
    plan_out[2] = s5 ? plan.s5_pos_bias : 0u;
    plan_out[3] = s5 ? plan.s5plan.fifo_cap : kScan2FifoCap;
    return GFT_OK;
} GFT_CATCH(nullptr)

int gft_debug_host_solve(const uint32_t* words, uint64_t len, const uint32_t* slots, const uint64_t* list_off,
                         const int64_t* positions, uint32_t n_lists, int* out) try {
    if (!words || !out || (n_lists && (!slots || !list_off))) return GFT_E_INVALID;
    uint32_t n_slots = 0;
    for (uint64_t i = 0; i < len; i++)
        if ((words[i] >> 28) == GFT_OP_UNIT) n_slots = std::max(n_slots, (words[i] & GFT_SLOT_MASK) + 1);
    ProgramTraits tr;
    std::string err;
    const int rc = check_program(words, len, n_slots, 0, tr, err);
    if (rc) return rc;
    SlotLists m;
    for (uint32_t k = 0; k < n_lists; k++) {
        std::vector<int64_t>& v = m[slots[k]];       // (a key may carry an empty list: expression_test.go:29-33)
        for (uint64_t i = list_off[k]; i < list_off[k + 1]; i++) v.push_back(positions[i]);
    }
    *out = host_solve(words, len, m) ? 1 : 0;
    return GFT_OK;
} GFT_CATCH(nullptr)

int gft_profile_enable(gft_engine* e, int on) try {
    if (!e) return GFT_E_INVALID;
    GFT_LOCK(e);
    e->profiling = on == 2 ? 2 : on != 0;
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

int gft_profile_reset(gft_engine* e) try {
    if (!e) return GFT_E_INVALID;
    GFT_LOCK(e);
    if (e->device < 0) return GFT_OK;
    DeviceGuard g(e->device);
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    for (auto& kv : e->prof) {
        for (auto& p : kv.second.ev) { e->prof_pool.push_back(p.first); e->prof_pool.push_back(p.second); }
        kv.second.ev.clear();
    }
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

int gft_profile_read(gft_engine* e, const char* name, double* total_ms, uint64_t* launches) try {
    if (!e || !name || !total_ms || !launches) return GFT_E_INVALID;
    GFT_LOCK(e);
    *total_ms = 0; *launches = 0;
    if (e->device < 0) return fail(e, GFT_E_HIP, "no HIP device available");
    DeviceGuard g(e->device);
    HIP_TRY(hipStreamSynchronize(e->stream), "sync");
    auto it = e->prof.find(name);
    if (it == e->prof.end()) return GFT_OK;
    for (auto& p : it->second.ev) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, p.first, p.second), "event elapsed");
        *total_ms += ms;
    }
    *launches = it->second.ev.size();
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

}  // extern "C"

// =====================================================================================================================
// Multi-device handles: one process, one host thread + stream per device, tables replicated,
// contiguous document ranges of near-equal text bytes, and -- for device-resident shards -- one RCCL gather of the
// bitmaps to the first device.  The Go side keeps calling finder.NewFinder(&GpuEngine{...}): the
// fan-out lives behind the same gft_engine handle.
// =====================================================================================================================
#include <dlfcn.h>
#include <rccl/rccl.h>

namespace {

// RCCL is bound at run time (dlopen): libgft.so itself does not depend on it, and a process that already carries a
// copy (PyTorch does) shares that one
struct RcclApi {
    ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    void* lib = nullptr;
    bool ok() const { return CommInitAll && CommDestroy && GroupStart && GroupEnd && Send && Recv && GetErrorString; }
};
RcclApi& rccl_api() {
    static RcclApi api;
    static std::once_flag once;
    std::call_once(once, [] {
        for (const char* name : {"librccl.so.1", "librccl.so"}) {
            api.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (api.lib) break;
        }
        if (!api.lib) return;
        api.CommInitAll = (decltype(api.CommInitAll))dlsym(api.lib, "ncclCommInitAll");
        api.CommDestroy = (decltype(api.CommDestroy))dlsym(api.lib, "ncclCommDestroy");
        api.GroupStart = (decltype(api.GroupStart))dlsym(api.lib, "ncclGroupStart");
        api.GroupEnd = (decltype(api.GroupEnd))dlsym(api.lib, "ncclGroupEnd");
        api.Send = (decltype(api.Send))dlsym(api.lib, "ncclSend");
        api.Recv = (decltype(api.Recv))dlsym(api.lib, "ncclRecv");
        api.GetErrorString = (decltype(api.GetErrorString))dlsym(api.lib, "ncclGetErrorString");
    });
    return api;
}

std::vector<gft_engine*> all_engines(gft_engine* e) {
    std::vector<gft_engine*> v{e};
    v.insert(v.end(), e->peers.begin(), e->peers.end());
    return v;
}

// behind a call that every device ran its share of: device 0's own verdict is this handle's, the peers' are OR-ed in
void or_peer_verdicts(gft_engine* e) {
    for (gft_engine* g : e->peers) e->reported.nonascii = e->reported.nonascii || g->reported.nonascii;
}

// contiguous document ranges of near-equal text bytes: device i owns documents [cut[i], cut[i+1])
void split_by_bytes(const uint64_t* doc_off, uint64_t n_docs, size_t n, std::vector<uint64_t>& cut) {
    cut.assign(n + 1, n_docs);
    cut[0] = 0;
    const uint64_t base = n_docs ? doc_off[0] : 0, total = n_docs ? doc_off[n_docs] - base : 0;
    for (size_t i = 1; i < n; i++) {
        const uint64_t target = base + (uint64_t)((unsigned __int128)total * i / n);
        uint64_t c = (uint64_t)(std::lower_bound(doc_off, doc_off + n_docs + 1, target) - doc_off);
        cut[i] = std::min(std::max(c, cut[i - 1]), n_docs);
    }
}

// run f(i, engine_i) for every device, each on its own host thread (the caller's thread takes device 0); the first
// failure's code and message become the handle's
template <class F>
int fan_out(gft_engine* e, F f) {
    const std::vector<gft_engine*> eng = all_engines(e);
    std::vector<int> rc(eng.size(), GFT_OK);
    std::vector<std::thread> th;
    th.reserve(eng.size());
    {
        JoinAll joined(th);                  // (also when a thread could not be started, or device 0's share threw)
        // a thread's body never lets an exception out (that would be std::terminate): it becomes the device's status
        auto guarded = [&](size_t i) noexcept {
            try { rc[i] = f(i, eng[i]); } catch (...) { rc[i] = translate_exception(&eng[i]->err); }
        };
        struct InMulti { gft_engine* e; explicit InMulti(gft_engine* e_) : e(e_) { e->in_multi = true; } ~InMulti() { e->in_multi = false; } };
        for (size_t i = 1; i < eng.size(); i++) th.emplace_back(guarded, i);
        InMulti im(e);
        guarded(0);
    }
    for (size_t i = 0; i < eng.size(); i++)
        if (rc[i]) {
            if (i) e->err = "device " + std::to_string(eng[i]->device) + ": " + eng[i]->err;
            return rc[i];
        }
    return GFT_OK;
}

void destroy_multi(gft_engine* e) {
    if (!e->comms.empty() && rccl_api().ok())
        for (void* c : e->comms) (void)rccl_api().CommDestroy((ncclComm_t)c);
    e->comms.clear();
    for (gft_engine* p : e->peers) gft_engine_destroy(p);
    e->peers.clear();
}

int replicate_tables(gft_engine* e, uint32_t flags) {
    // the compiled tables are copied, not compiled again; every device uploads its own copy
    std::vector<std::thread> th;
    std::vector<int> rc(e->peers.size(), GFT_OK);
    th.reserve(e->peers.size());
    {
        JoinAll joined(th);
        for (size_t i = 0; i < e->peers.size(); i++)
            th.emplace_back([&, i]() noexcept {
                gft_engine* p = e->peers[i];
                try {
                    GFT_LOCK(p);
                    TableSet copy = e->tables;
                    rc[i] = install_tables(p, std::move(copy), flags);
                } catch (...) { rc[i] = translate_exception(&p->err); }
            });
    }
    for (size_t i = 0; i < rc.size(); i++)
        if (rc[i]) { e->err = "device " + std::to_string(e->peers[i]->device) + ": " + e->peers[i]->err; return rc[i]; }
    return GFT_OK;
}

int multi_build(gft_engine* e, const uint8_t* terms_blob, const uint64_t* term_off, uint32_t n_terms, uint32_t flags) {
    e->in_multi = true;
    const int rc = gft_build(e, terms_blob, term_off, n_terms, flags);
    e->in_multi = false;
    return rc ? rc : replicate_tables(e, flags);
}

int multi_import_tables(gft_engine* e, const uint8_t* blob, uint64_t len) {
    e->in_multi = true;
    const int rc = gft_import_tables(e, blob, len);
    e->in_multi = false;
    return rc ? rc : replicate_tables(e, e->build_flags);
}

int multi_set_programs(gft_engine* e, const uint32_t* prog_words, const uint64_t* prog_off, uint32_t n_exprs, uint32_t n_extra) {
    return fan_out(e, [&](size_t, gft_engine* g) { return gft_set_programs(g, prog_words, prog_off, n_exprs, n_extra); });
}

// caller-supplied matches of the documents [a, b): the same arrays, offsets rebased
struct ExtraSlice {
    std::vector<uint64_t> off;
    gft_extra_matches x{nullptr, nullptr, nullptr};
    const gft_extra_matches* ptr = nullptr;
    void set(const gft_extra_matches* extra, uint64_t a, uint64_t b) {
        if (!(extra && extra->off)) return;
        off.assign(extra->off + a, extra->off + b + 1);
        const uint64_t base = off[0];
        for (auto& o : off) o -= base;
        x.off = off.data(); x.slot = extra->slot + base; x.pos = extra->pos + base;
        ptr = &x;
    }
};

int multi_process(gft_engine* e, const uint8_t* text_blob, const uint64_t* doc_off, uint64_t n_docs, uint32_t flags,
                  const gft_extra_matches* extra, uint32_t* hit_bitmap) {
    const size_t n = e->peers.size() + 1;
    // (an empty batch may come without offsets, as on a single device: every shard then is [0, 0) of this one entry)
    static const uint64_t kNoDocs[1] = {0};
    if (n_docs == 0) doc_off = kNoDocs;
    split_by_bytes(doc_off, n_docs, n, e->shard_cut);
    const uint64_t words = (e->n_exprs + 31) / 32;
    e->reported.nonascii = false;
    const int rc = fan_out(e, [&](size_t i, gft_engine* g) {
        const uint64_t a = e->shard_cut[i], b = e->shard_cut[i + 1];
        std::vector<uint64_t> off(doc_off + a, doc_off + b + 1);        // this shard's documents, offsets from its first byte
        const uint64_t base = off[0];
        for (auto& o : off) o -= base;
        ExtraSlice xs;
        xs.set(extra, a, b);
        return gft_process(g, text_blob + base, off.data(), b - a, flags, xs.ptr, hit_bitmap ? hit_bitmap + a * words : nullptr);
    });
    or_peer_verdicts(e);
    return rc;
}

int multi_process_again(gft_engine* e, uint64_t n_docs, const gft_extra_matches* extra, uint32_t* hit_bitmap) {
    const size_t n = e->peers.size() + 1;
    if (e->shard_cut.size() != n + 1 || e->shard_cut.back() != n_docs || !n_docs)
        return fail(e, GFT_E_INVALID, "gft_process_again: no scan of these documents to reuse");
    const uint64_t words = (e->n_exprs + 31) / 32;
    return fan_out(e, [&](size_t i, gft_engine* g) {
        const uint64_t a = e->shard_cut[i], b = e->shard_cut[i + 1];
        if (a == b) return (int)GFT_OK;
        ExtraSlice xs;
        xs.set(extra, a, b);
        return gft_process_again(g, b - a, xs.ptr, hit_bitmap ? hit_bitmap + a * words : nullptr);
    });
}

int multi_scan(gft_engine* e, const uint8_t* text_blob, const uint64_t* doc_off, uint64_t n_docs, uint32_t flags, gft_matches* out) {
    const size_t n = e->peers.size() + 1;
    static const uint64_t kNoDocs[1] = {0};
    if (n_docs == 0) doc_off = kNoDocs;                  // (see multi_process)
    std::vector<uint64_t> cut;
    split_by_bytes(doc_off, n_docs, n, cut);
    std::vector<gft_matches> part(n);
    int rc = fan_out(e, [&](size_t i, gft_engine* g) {
        const uint64_t a = cut[i], b = cut[i + 1];
        std::vector<uint64_t> off(doc_off + a, doc_off + b + 1);
        const uint64_t base = off[0];
        for (auto& o : off) o -= base;
        return gft_scan(g, text_blob + base, off.data(), b - a, flags, &part[i]);
    });
    if (rc) return rc;
    // the shards' CSRs one behind the other (device 0's own result lives in this handle's vectors: copied out first)
    uint64_t total = 0;
    for (const auto& p : part) total += p.n_matches;
    std::vector<uint64_t> mo(n_docs + 1, 0);
    std::vector<uint32_t> ti((size_t)total), po((size_t)total);
    uint64_t at = 0;
    for (size_t i = 0; i < n; i++) {
        const uint64_t a = cut[i], nd = cut[i + 1] - a;
        for (uint64_t d = 0; d <= nd; d++) mo[a + d] = at + part[i].match_off[d];
        if (part[i].n_matches) {
            memcpy(ti.data() + at, part[i].term_id, part[i].n_matches * 4);
            memcpy(po.data() + at, part[i].pos, part[i].n_matches * 4);
        }
        at += part[i].n_matches;
    }
    e->h_match_off.swap(mo); e->h_term.swap(ti); e->h_pos.swap(po);
    or_peer_verdicts(e);
    out->n_docs = n_docs; out->n_matches = total;
    out->match_off = e->h_match_off.data(); out->term_id = e->h_term.data(); out->pos = e->h_pos.data();
    return GFT_OK;
}

}  // namespace

extern "C" {

int gft_engine_create_multi(gft_engine** out, const int* devices, int n_devices) try {
    if (!out || n_devices < 0 || (n_devices && !devices)) return GFT_E_INVALID;
    *out = nullptr;
    std::vector<int> devs(devices, devices + n_devices);
    if (devs.empty()) {
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess) count = 0;
        for (int d = 0; d < count; d++) devs.push_back(d);
        if (devs.empty()) devs.push_back(0);       // (gft_engine_create reports the missing device)
    }
    gft_engine* e = nullptr;
    int rc = gft_engine_create(&e, devs[0]);
    *out = e;
    if (rc) return rc;
    for (size_t i = 1; i < devs.size(); i++) {
        gft_engine* p = nullptr;
        rc = gft_engine_create(&p, devs[i]);
        if (rc) {
            e->err = "device " + std::to_string(devs[i]) + ": " + (p ? p->err : std::string("cannot create an engine"));
            if (p) gft_engine_destroy(p);
            return rc;
        }
        e->peers.push_back(p);
    }
    // RCCL communicators over xGMI for the device-resident entry point -- only when the devices are distinct (a list
    // that names one device twice is a test configuration: the gather is then plain device-to-device copies)
    std::vector<int> uniq(devs);
    std::sort(uniq.begin(), uniq.end());
    const bool distinct = std::adjacent_find(uniq.begin(), uniq.end()) == uniq.end();
    // GFT_RCCL_SELF=1: a list that names ONE device several times gets a communicator of one rank, and the gather moves every
    // further shard's bitmap with a grouped ncclSend / ncclRecv of that rank to itself -- the same dlopen, the same bound
    // entry points, the same group and stream ordering as the N-device gather, on the one GPU a test box has
    const char* self_env = getenv("GFT_RCCL_SELF");
    e->rccl_self = devs.size() > 1 && uniq.front() == uniq.back() && self_env && self_env[0] == '1';
    if (devs.size() > 1 && (distinct || e->rccl_self)) {
        RcclApi& api = rccl_api();
        if (!api.ok()) {
            e->rccl_self = false;
            e->err = "RCCL (librccl.so) could not be loaded: bitmaps will be gathered by device-to-device copies";
            return GFT_W_NO_RCCL;
        }
        std::vector<ncclComm_t> comms(e->rccl_self ? 1 : devs.size());
        DeviceGuard dg(devs[0]);
        const ncclResult_t r = api.CommInitAll(comms.data(), (int)comms.size(), devs.data());
        if (r != ncclSuccess) {
            // the handle is complete without communicators, but the caller is TOLD that its gathers are not RCCL's
            e->rccl_self = false;
            e->err = std::string("ncclCommInitAll: ") + api.GetErrorString(r) + " (bitmaps will be gathered by device-to-device copies)";
            return GFT_W_NO_RCCL;
        }
        for (ncclComm_t c : comms) e->comms.push_back((void*)c);
    }
    return GFT_OK;
} GFT_CATCH(nullptr)

int gft_n_devices(const gft_engine* e) { return e ? (int)e->peers.size() + 1 : 0; }
const char* gft_gather_mode(const gft_engine* e) { return !e || e->peers.empty() ? "" : e->comms.empty() ? "copy" : "rccl"; }

gft_engine* gft_device_engine(gft_engine* e, int i) {
    if (!e || i < 0 || i > (int)e->peers.size()) return nullptr;
    return i == 0 ? e : e->peers[(size_t)i - 1];
}

int gft_split_docs(const gft_engine* e, const uint64_t* doc_off, uint64_t n_docs, uint64_t* cut) try {
    if (!e || !cut || (n_docs && !doc_off)) return GFT_E_INVALID;
    std::vector<uint64_t> c;
    split_by_bytes(doc_off, n_docs, e->peers.size() + 1, c);
    memcpy(cut, c.data(), c.size() * 8);
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

int gft_process_device_multi(gft_engine* e, const uint8_t* const* d_text, const uint64_t* const* d_doc_off, const uint64_t* n_docs,
                             uint32_t flags, uint32_t* d_bitmap_root) try {
    if (!e || !d_text || !d_doc_off || !n_docs) return e ? fail(e, GFT_E_INVALID, "null argument") : GFT_E_INVALID;
    GFT_LOCK(e);
    if (!e->built) return fail(e, GFT_E_NOT_BUILT, "gft_build has not been called");
    if (!e->have_programs) return fail(e, GFT_E_NOT_BUILT, "gft_set_programs has not been called");
    const std::vector<gft_engine*> eng = all_engines(e);
    const size_t n = eng.size();
    const uint64_t words = (e->n_exprs + 31) / 32;
    std::vector<uint64_t> first(n + 1, 0);
    for (size_t i = 0; i < n; i++) first[i + 1] = first[i] + n_docs[i];
    if (first[n] * words && !d_bitmap_root) return fail(e, GFT_E_INVALID, "null bitmap");
    // every device solves its shard into its own bitmap (device 0 straight into its slice of the result) ...
    int rc = fan_out(e, [&](size_t i, gft_engine* g) {
        uint32_t* dst = d_bitmap_root;
        if (i) {
            GFT_LOCK(g);
            DeviceGuard dg(g->device);
            if (g->d_bitmap.ensure(std::max<uint64_t>(n_docs[i] * words, 1) * 4) != hipSuccess) return fail(g, GFT_E_HIP, "bitmap alloc");
            dst = g->d_bitmap.as<uint32_t>();
        }
        return gft_process_device(g, d_text[i], d_doc_off[i], n_docs[i], flags, nullptr, dst);
    });
    if (rc) return rc;
    // ... then ONE exchange step: the shards' bitmaps to the first device, ncclSend / ncclRecv in one group over xGMI
    // (plain device-to-device copies when there is no communicator)
    if (n > 1 && words) {
        RcclApi& api = rccl_api();
        if (!e->comms.empty() && api.ok()) {
            DeviceGuard dgr(e->device);
            ncclResult_t r = api.GroupStart();
            for (size_t i = 1; i < n && r == ncclSuccess; i++) {
                if (!n_docs[i]) continue;
                // (one rank for all shards under GFT_RCCL_SELF: peer 0 on communicator 0, both halves on the root's stream --
                // the shard's stream was drained when its gft_process_device returned)
                const int from = e->rccl_self ? 0 : (int)i;
                ncclComm_t send_comm = (ncclComm_t)e->comms[e->rccl_self ? 0 : i];
                hipStream_t send_stream = e->rccl_self ? e->stream : eng[i]->stream;
                r = api.Recv(d_bitmap_root + first[i] * words, n_docs[i] * words, ncclUint32, from, (ncclComm_t)e->comms[0], e->stream);
                if (r == ncclSuccess)
                    r = api.Send(eng[i]->d_bitmap.p, n_docs[i] * words, ncclUint32, 0, send_comm, send_stream);
            }
            const ncclResult_t r2 = api.GroupEnd();
            if (r != ncclSuccess || r2 != ncclSuccess)
                return fail(e, GFT_E_HIP, std::string("RCCL gather: ") + api.GetErrorString(r != ncclSuccess ? r : r2));
            for (gft_engine* g : eng) {
                DeviceGuard dg(g->device);
                HIP_TRY(hipStreamSynchronize(g->stream), "RCCL gather");
            }
        } else {
            DeviceGuard dg(e->device);
            for (size_t i = 1; i < n; i++)
                if (n_docs[i]) HIP_TRY(hipMemcpyAsync(d_bitmap_root + first[i] * words, eng[i]->d_bitmap.p, n_docs[i] * words * 4, hipMemcpyDeviceToDevice, e->stream), "bitmap gather");
            HIP_TRY(hipStreamSynchronize(e->stream), "bitmap gather");
        }
    }
    or_peer_verdicts(e);
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

}  // extern "C"
