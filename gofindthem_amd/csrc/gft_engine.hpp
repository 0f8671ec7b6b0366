// gft_engine.hpp -- what the files behind the C ABI of include/gft.h share: the engine handle, its device buffers, the
// guards and macros of an entry point, and the internal functions that cross files (namespace gft::api).  Internal: it is
// not installed beside include/gft.h, and only the gft_*.cpp orchestration files include it (file map: DESIGN.md 1).
#pragma once
#include "../../include/gft.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "batch_verdict.hpp"
#include "copy_pool.hpp"
#include "gft_guard.hpp"
#include "gft_kernels.hpp"
#include "program_set.hpp"
#include "solve_plan.hpp"
#include "table_set.hpp"

namespace gft::api {

// Device memory that grows and never shrinks, and frees itself with its owner (under the owner's DeviceGuard:
// gft_engine_destroy)
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
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

}  // namespace gft::api

struct gft_engine {
    using DevBuf = gft::api::DevBuf;
    int device = 0;
    hipStream_t stream = nullptr;
    // host -> device staging of large caller buffers (gft_staging.cpp): two pinned bounce buffers, filled by a few copy
    // threads while the previous one is on the wire (a hipMemcpy from pageable memory stages through one thread)
    struct Staging {
        void* pin[2] = {nullptr, nullptr};
        hipEvent_t pin_ev[2] = {nullptr, nullptr};
        std::unique_ptr<gft::CopyPool> copy_pool;   // the threads that fill / empty the bounce buffers (created with the first large copy)
    } staging;
    uint64_t* pin_rb = nullptr;            // pinned landing place of the per-batch read-back of the control block
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
    gft::Scan5Tables s5;
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
    gft::api::PoolState pool;
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
    uint32_t solve_unit_entries = 0;       // learned.unit_entries as the last scan_pipeline found it: what that batch's solver plans with
    uint32_t last_pf_terms = 0;            // the prefetch depth of the last solver launch (gft_debug_last_solve_pf)
    const char* last_unit_route = "";      // how scan_pipeline made the unit table of the last batch it launched (gft_debug_last_unit_route)
    // gft_process_device_begin / _end: up to two batches enqueued, their read-backs landing in pinned slots of their own
    struct Pending {
        bool done = false;                 // completed inside begin (a batch that could not be deferred): rc is its status
        int rc = 0;
        const uint8_t* d_text = nullptr; const uint64_t* d_doc_off = nullptr; uint64_t n_docs = 0; uint32_t flags = 0;
        uint32_t* d_bitmap = nullptr;
        gft::ScanLaunch launch;
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
    struct UniqueBufs { DevBuf first, cnt, off, term; } d_uq;       // GFT_SCAN_UNIQUE: per-workgroup first-occurrence rows, unique CSR
    struct RuneBufs { DevBuf cnt, base, starts, prefix; } d_rn;     // GFT_POS_RUNES: blocks per document, their rune starts, prefix sums
    std::vector<uint64_t> h_match_off;
    std::vector<uint32_t> h_term, h_pos;
    // sparse results (gft_compact.hip): a label per expression (gft_set_expr_labels); the compaction's scratch -- counts and
    // scan partials of its own, so that it may run beside batches in flight --, and the CSR of gft_process_sparse
    bool have_labels = false;
    std::vector<uint32_t> h_labels;
    DevBuf d_labels;
    struct SparseBufs {
        DevBuf cnt, partial, row_off, idx, label;
        std::vector<uint64_t> h_row_off;
        std::vector<uint32_t> h_expr_idx, h_label, h_bitmap;
    } sparse;
    // strings.ToLower on the device (gft_tolower.hip): the mapping table (uploaded with the first call), a unit table, counts
    // and scan partials of its own, and the lowered batch the finder scans again (gft_lower_owned)
    struct LowerBufs {
        bool table_up = false;
        DevBuf page, delta, doc_units, unit_base, units, partial, unit_cnt, unit_out, ctl, text, off;
    } d_lw;

    // a blob cut into line documents (gft_split.hip): tile summaries, the carry in front of every tile, counts, their prefix
    // sums and scan partials of its own
    struct SplitBufs { DevBuf sums, carry, cnt, base, partial; } d_split;

    // the documents that matched, gathered into one blob (gft_select.hip): the mask, the lengths and marks of a batch, their
    // prefix sums, scan partials and read-back words of its own, and the compact offsets the copy pass searches
    struct SelectBufs { DevBuf want, len, sel, pos, rank, partial, ctl, c_off, c_src; } d_select;

    // context lines round the documents that matched (gft_context.hip): the mask, the marks of a batch (then its group heads), the
    // tiles' ballot words with what they say to the other tiles, the carries of the tiles and of the carry blocks, the keep flags
    // and lengths, the three prefix sums with scan partials and read-back words of its own, and the compact offsets the select's
    // copy pass searches
    struct ContextBufs { DevBuf want, sel, len, keep, word_sel, word_fence, sum, carry, part, pos, rank, grank, partial, ctl, c_off, c_src; } d_context;

    // documents routed to per-bucket runs of one blob (gft_route.hip): the masks, the member words and lengths of a batch, the
    // (bucket, tile) counts with their prefix sums, the tiles' bytes, scan partials and read-back words of its own, and the
    // entries' lengths and compact offsets the select's copy pass searches
    struct RouteBufs { DevBuf masks, member, len, cnt, tile_bytes, base, partial, ctl, ent_len, c_off, c_src; } d_route;

    // hit spans and redaction (gft_spans.hip): the witness table of the installed programs (witness_terms.hpp; compiled and
    // uploaded by the first spans call after a gft_set_programs, dropped with the programs), the mask, the marks of a batch's
    // matches with their prefix sums and scan partials; the redaction's span addresses and its flag word
    struct SpanBufs {
        bool wit_ready = false;
        DevBuf wit_off, wit_expr, want, keep, rank, partial, dst, ctl;
    } d_spans;

    // lowered spans mapped back to the source text (gft_lowermap.hip): the pieces' offset table, the lowered offsets the count
    // passes want, the mapped spans between the check and the write pass, the flag word
    struct LowerMapBufs { DevBuf tab, off, mapped, ctl; } d_lmap;

    // excerpts round the hit spans (gft_excerpt.hip): every span's window, document, suffix minimum, head mark and share of its
    // excerpt's length, the tiles' minima and carries, the two prefix sums with scan partials and read-back words of their own,
    // and the compact offsets the select's copy pass searches
    struct ExcerptBufs {
        DevBuf ws, we, sdoc, smin, head, share, tmin, carry, rank, pos, partial, ctl, c_off, c_src;
        uint64_t* pin = nullptr;           // pinned landing place of the control block's read-backs (freed with the handle)
    } d_excerpt;

    // highlight (gft_mark.hip): the run passes work in the excerpt's buffers; the insertion list and the marker block are its own
    struct MarkBufs { DevBuf q, marks; } d_mark;

    // replace (gft_replace.hip): the run passes work in the excerpt's buffers; every run's smallest id, the heads' replacement
    // lengths and their prefix sum, the call's copies of the key map and the table, and the plan are its own
    struct ReplaceBufs { DevBuf rid, pl, ppos, key_rep, rep_off, tab, at, delta, len, roff; } d_replace;

    // term statistics and column counts (gft_stats.hip): the check pass's flag words and the workgroups' bitset rows for
    // dictionaries whose bitset leaves LDS
    struct StatsBufs { DevBuf ctl, rows; } d_stats;

    // the kept matches of a batch call with a hit bitmap, as a span CSR (gft_term_list.cpp): batch_term_list fills it from
    // gft_hit_spans_device or its whole-word twin for gft_batch_term_stats_device, gft_batch_top_docs_device and their twins, whose
    // consumers read off and term (the starts are what the spans call asks for with any cap).  It holds until the next such call.
    struct KeptBufs { DevBuf off, start, term; } d_kept;

    // scores, the top list and the gather by index list (gft_rank.hip): the control block, the call's copy of the weights, the
    // workgroups' bitset rows of the distinct mode, the select's histograms, the place tiles' counts with their prefix sums and scan
    // partials, the candidates; the gather's lengths and the compact arrays the select's copy pass searches; the scores of
    // gft_batch_top_docs_device when the caller asks for none
    struct RankBufs {
        DevBuf ctl, weights, rows, hist, tile_gt, tile_eq, gt_pos, eq_pos, partial, cand_score, cand_idx, len, c_off, c_src, score;
    } d_rank;

    // whole-word matching (gft_words.hip): the class table (uploaded with the first call), the check pass's flag words, the marks of
    // a list's entries with their prefix sums and scan partials; the kept matches of gft_scan_words_device / gft_process_words_device
    // (off, pos, term), the spans gft_hit_spans_words_device filters (the filter's input, which its output must not overlap)
    struct WordBufs {
        bool table_up = false;
        DevBuf tab_row, tab_bits, ctl, keep, rank, partial, off, pos, term, span_off, span_start, span_len, span_term;
    } d_words;

    // rule evaluation for records (gft_rules.hip): the installed set's shape and its arrays on the device, the leaf bitmap and
    // the tag rows of a batch, the flag words, staging for the host-pointer entry points
    struct RuleBufs {
        uint64_t serial = 0;               // 0: none installed
        uint32_t n_fields = 0, n_tags = 0, n_exprs = 0, n_rules = 0, n_units = 0, max_depth = 0, field_words = 0;
        DevBuf expr_tag, masks, units, prog, prog_off, leaf_bitmap, tag_rows, flags, stage[6];
        DevBuf valid;                      // [field_words] the set's validity mask (gft_tags.hip)
    } d_rules;

    // tag entries of a record batch (gft_tags.hip): counts, leaf offsets, scan partials and flag words of their own -- apart from
    // the compaction's scratch and the rule kernels' buffers --, and the arrays of the owned form (rules_tag_entries_owned)
    struct TagBufs {
        DevBuf cnt, leaf_ent_off, partial, flags, row_off, ent_field, ent_expr;
    } d_tags;

    // the result document of a batch's rule rows (gft_result.hip): the installed fragment table (rules_json.hpp), counts, prefix
    // sums, scan partials and flag words of their own, the hole lengths and the text of the owned form (rules_json_owned)
    struct ResultBufs {
        uint64_t serial = 0;               // 0: no table installed
        uint32_t n_exprs = 0;
        DevBuf rule_first, name_off, name_len, expr_off, expr_len, blob, cnt, scan, partial, flags, hole_len, out_off, text;
    } d_result;

    // the tag result document of a record batch (gft_tagdoc.hip): the installed slot and field tables (tags_json.hpp), the slot
    // rows of a batch, the staged leaf fields and record offsets (tags_json_stage), counts, prefix sums, scan partials and flag
    // words of their own, the hole lengths and the text of the owned form (tags_json_owned)
    struct TagDocBufs {
        uint64_t slot_serial = 0, field_serial = 0;    // 0: no table installed
        uint32_t n_exprs = 0, SW = 0, n_tags = 0, n_fields = 0;
        DevBuf src_off, src_expr, slot_off, slot_len, tag_word, tag_words, tag_off, tag_len, slot_blob;
        DevBuf field_rank, field_off, field_len, valid, field_blob;
        DevBuf slot_rows, leaf_field, rec_off, cnt, scan, partial, flags, hole_len, out_off, text;
        bool staged = false;                           // slot_rows, leaf_field and rec_off hold a batch of ...
        uint64_t staged_records = 0, staged_leaves = 0;
    } d_tagdoc;

    // JSON documents decoded on the device (gft_json.hip): the installed schema trie, the counts and prefix sums of a batch, the
    // record arrays of gft_group_process_jsons_device, staging for the host-pointer entry point
    struct JsonBufs {
        uint64_t serial = 0;               // 0: no trie installed
        uint32_t n_nodes = 0, table_mask = 0, max_key_len = 0;
        DevBuf nodes, keys, table, cnt_leaves, cnt_text, text_off, partial, flags, rec_off, leaf_field, leaf_off, text, blob, doc_off, status, rows;
        DevBuf paths;                      // discovery (k_json_paths): counters, hash set, path offsets, pool; allocated once
    } d_json;

    // profiling
    int profiling = 0;                     // gft_profile_enable: 0 off, 1 every category, 2 the scan kernel only
    std::vector<hipEvent_t> prof_pool;     // events given back by gft_profile_reset
    std::map<std::string, gft::api::ProfCat> prof;
};

#define GFT_LOCK(e) std::lock_guard<std::recursive_mutex> _gft_lock((e)->mu)

#define HIP_TRY(expr, what)                                             \
    do {                                                                \
        hipError_t _h = (expr);                                         \
        if (_h != hipSuccess) return gft::api::fail_hip(e, _h, what);   \
    } while (0)

namespace gft::api {

inline int fail(const gft_engine* e, int code, const std::string& msg) {
    e->err = msg;
    return code;
}
inline int fail_hip(const gft_engine* e, hipError_t h, const char* what) {
    e->err = std::string(what) + ": " + hipGetErrorString(h);
    return GFT_E_HIP;
}

// a work buffer grown on demand to at least `bytes` (and 16); the texts of its two failures: GFT_E_NOMEM's message, and what
// fail_hip names for any other error
struct RoomTexts { const char* nomem; const char* alloc; };
inline int room(const gft_engine* e, DevBuf& b, uint64_t bytes, const RoomTexts& t) {
    const hipError_t h = b.ensure(std::max<uint64_t>(bytes, 16));
    if (h == hipErrorOutOfMemory) { (void)hipGetLastError(); return fail(e, GFT_E_NOMEM, t.nomem); }
    return h == hipSuccess ? (int)GFT_OK : fail_hip(e, h, t.alloc);
}

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

// a scan entry point's last act on every way out behind its scan: the batch's verdict becomes the handle's
struct Publish {
    gft_engine* e; const BatchVerdict& v;
    ~Publish() { e->reported = v; }
};

template <class T>
int upload(gft_engine* e, DevBuf& buf, const std::vector<T>& v, const char* what) {
    HIP_TRY(buf.ensure(std::max<size_t>(v.size() * sizeof(T), 16)), what);
    if (!v.empty()) HIP_TRY(hipMemcpyAsync(buf.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, e->stream), what);
    return GFT_OK;
}

// ---- gft_api.cpp -------------------------------------------------------------------------------------------------------
// what plan_scan is told (table_set.hpp): GFT_SCAN_KERNEL and the GFT_SCAN5_* switches
ScanOptions scan_options();
int install_tables(gft_engine* e, TableSet&& set, uint32_t flags);
// gft_process_device_begin / _end: no batch in flight is still to be completed (the synchronous entry points may run)
bool pend_settled(const gft_engine* e);
// What an entry point needs of the handle before it starts, tested in this order; the first that fails gives its code and
// message (who: the prefix of the in-flight message, for the entry points that name themselves there)
enum : unsigned { kNeedDevice = 1, kNeedBuilt = 2, kNeedPrograms = 4, kNeedSettled = 8 };
int check_ready(const gft_engine* e, unsigned need, const char* who = nullptr);

// ---- gft_pipeline.cpp --------------------------------------------------------------------------------------------------
extern const bool kExtraKernels;           // this build carries gft_scan2.hip / gft_scan4.hip (GFT_EXTRA_KERNELS)
// The device pipeline shared by scan and process.  defer != nullptr: the launch may be deferred -- the caller reads the
// control block back itself after its last kernel and hands it to deferred_interpret
int scan_pipeline(gft_engine* e, const uint8_t* d_text, const uint64_t* d_doc_off, uint64_t n_docs, uint32_t flags, bool need_csr,
                  BatchVerdict& v, const uint64_t* h_doc_off = nullptr, ScanLaunch* defer = nullptr);
int deferred_interpret(gft_engine* e, const uint64_t* raw, const ScanLaunch& L, BatchVerdict& v, bool* again);
int refine_nonascii(gft_engine* e, const uint8_t* d_text, const uint64_t* d_doc_off, uint64_t n_docs, uint32_t flags, BatchVerdict& v);
int unique_pipeline(gft_engine* e, uint64_t n_docs, uint64_t* n_matches);
int rune_pipeline(gft_engine* e, const uint8_t* d_text, const uint64_t* d_doc_off, uint64_t n_docs, uint64_t n_matches);
int solve_pipeline(gft_engine* e, uint64_t n_docs, const gft_extra_matches* d_extra, uint32_t* d_bitmap);
// what the host solves (host_solve.hpp)
struct HostPlan {
    bool all_docs = false;                     // some expression is beyond the device solver's limits: every document
    std::vector<uint64_t> irregular;           // documents in which a slot read by an INORD group may have a non-ascending list
    bool empty() const { return !all_docs && irregular.empty(); }
};
void plan_host(const gft_engine* e, const gft_extra_matches* extra, uint64_t n_docs, HostPlan& plan);
int host_eval(gft_engine* e, const gft_extra_matches* extra, uint64_t n_docs, const HostPlan& plan, uint32_t* h_bitmap, uint32_t* d_bitmap);

// ---- gft_lower_api.cpp -------------------------------------------------------------------------------------------------
// the unit table of a batch, the count pass and the prefix sum of gft_to_lower_device into e->d_lw (units, unit_base, unit_out) and
// d_out_off; waits for the stream.  who: the entry point the refusals name; stage: NULL, or one gft_profile_read name for the
// count and the prefix instead of "lower_count" / "lower_scan"; text_range: NULL, or [2] for doc_off[0] and doc_off[n_docs]
int lower_count(gft_engine* e, const uint8_t* d_text, const uint64_t* d_doc_off, uint64_t n_docs, const uint8_t* d_out, uint64_t cap,
                uint64_t* d_out_off, uint64_t* n_units, uint64_t* total, const char* who, const char* stage = nullptr,
                uint64_t* text_range = nullptr);

// ---- gft_rank_api.cpp --------------------------------------------------------------------------------------------------
// the tail of gft_batch_top_docs_device and its words twin behind batch_term_list (which has tested k and the top arrays): the
// list's scores into d_score (NULL: a buffer of the engine's), then the top list of those scores, the select starting at the
// maximum the score pass found.  who: the entry point
int batch_top_tail(gft_engine* e, const char* who, const uint64_t* d_off, const uint32_t* d_term, uint64_t n_docs, uint32_t n_terms,
                   const uint32_t* weights, uint32_t flags, uint32_t k, uint64_t doc_base, uint64_t* d_score, uint64_t* d_top_idx,
                   uint64_t* d_top_score, uint64_t* n_top);

// ---- gft_staging.cpp ---------------------------------------------------------------------------------------------------
// device -> pageable host memory through the bounce buffers; synchronous: returns when dst holds the bytes
int d2h_staged(gft_engine* e, void* dst, const void* src, size_t bytes);
// a batch from host memory into e->d_text / e->d_doc_off (asynchronous: the caller drains the stream)
int stage_docs(gft_engine* e, const uint8_t* text_blob, const uint64_t* doc_off, uint64_t n_docs);

// ---- gft_multi.cpp: multi-device dispatch of the single-device entry points --------------------------------------------
void destroy_multi(gft_engine* e);
int multi_process(gft_engine* e, const uint8_t* text_blob, const uint64_t* doc_off, uint64_t n_docs, uint32_t flags,
                  const gft_extra_matches* extra, uint32_t* hit_bitmap);
int multi_process_again(gft_engine* e, uint64_t n_docs, const gft_extra_matches* extra, uint32_t* hit_bitmap);
int multi_scan(gft_engine* e, const uint8_t* text_blob, const uint64_t* doc_off, uint64_t n_docs, uint32_t flags, gft_matches* out);
int multi_set_programs(gft_engine* e, const uint32_t* prog_words, const uint64_t* prog_off, uint32_t n_exprs, uint32_t n_extra);
int multi_build(gft_engine* e, const uint8_t* terms_blob, const uint64_t* term_off, uint32_t n_terms, uint32_t flags);
int multi_import_tables(gft_engine* e, const uint8_t* blob, uint64_t len);

}  // namespace gft::api
