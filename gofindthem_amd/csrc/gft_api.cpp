// gft_api.cpp -- the C ABI of include/gft.h, the handle's side: engine create / destroy, stream and CU margin, the
// environment switches, table and program install, labels, the small getters, profiling, and the readiness check every
// entry point starts with.  The batch entry points are in gft_process.cpp, the kernel pipelines in gft_pipeline.cpp
// (DESIGN.md 1 has the file map).  Host orchestration only; there is no CPU fallback: every compute entry point needs
// a HIP device.
#include "gft_engine.hpp"

#include <cstdio>
#include <cstdlib>

using namespace gft;
using namespace gft::api;

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
    const long pf = num("GFT_SOLVE_PF_TERMS", 0);
    e->opt_solve.forced_pf = pf == 6 || pf == 12 ? (uint32_t)pf : 0u;
}

}  // namespace

namespace gft::api {

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

bool pend_settled(const gft_engine* e) {
    for (unsigned i = 0; i < e->pend_count; i++)
        if (!e->pend[(e->pend_head + i) % 2].done) return false;
    return true;
}

int check_ready(const gft_engine* e, unsigned need, const char* who) {
    if ((need & kNeedDevice) && e->device < 0) return fail(e, GFT_E_HIP, "no HIP device available");
    if ((need & kNeedBuilt) && !e->built) return fail(e, GFT_E_NOT_BUILT, "gft_build has not been called");
    if ((need & kNeedPrograms) && !e->have_programs) return fail(e, GFT_E_NOT_BUILT, "gft_set_programs has not been called");
    if ((need & kNeedSettled) && !pend_settled(e))
        return fail(e, GFT_E_INVALID, (who ? std::string(who) + ": " : std::string()) +
                                          "batches of gft_process_device_begin are in flight: gft_process_device_end (or _complete) first");
    return GFT_OK;
}

}  // namespace gft::api

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
    if (e->device < 0) {                   // (never allocated anything)
        destroy_multi(e);
        delete e;
        return;
    }
    DeviceGuard g(e->device);
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    for (auto& kv : e->prof)
        for (auto& p : kv.second.ev) { e->prof_pool.push_back(p.first); e->prof_pool.push_back(p.second); }
    for (hipEvent_t ev : e->prof_pool) (void)hipEventDestroy(ev);
    for (int k = 0; k < 2; k++) {
        if (e->staging.pin[k]) (void)hipHostFree(e->staging.pin[k]);
        if (k == 0 && e->pin_rb) (void)hipHostFree(e->pin_rb);
        if (e->staging.pin_ev[k]) (void)hipEventDestroy(e->staging.pin_ev[k]);
        if (e->pend[k].rb) (void)hipHostFree(e->pend[k].rb);
        if (e->pend[k].ev) (void)hipEventDestroy(e->pend[k].ev);
    }
    if (e->d_excerpt.pin) (void)hipHostFree(e->d_excerpt.pin);
    destroy_multi(e);
    // the device buffers free themselves with the engine, on its device; its own stream outlives them
    hipStream_t own = e->own_stream ? e->stream : nullptr;
    delete e;
    if (own) (void)hipStreamDestroy(own);
}

const char* gft_last_error(const gft_engine* e) { return e ? e->err.c_str() : "null engine"; }

int gft_set_stream(gft_engine* e, void* hip_stream) try {
    if (!e) return GFT_E_INVALID;
    GFT_LOCK(e);
    if (int rc = check_ready(e, kNeedDevice)) return rc;
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
    if (int rc = check_ready(e, kNeedDevice)) return rc;
    if (e->pend_count) return fail(e, GFT_E_INVALID, "batches are in flight (gft_process_device_end first)");
    e->cu_margin = margin;
    e->n_cus = e->n_cus_hw > margin ? e->n_cus_hw - margin : 1;
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

}  // extern "C"

namespace gft::api {

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
int install_tables(gft_engine* e, TableSet&& set, uint32_t flags) {
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
    e->d_spans.wit_ready = false;
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
    e->learned.unit_entries = 0;
    e->built = true;
    return GFT_OK;
}

}  // namespace gft::api

extern "C" {

int gft_build(gft_engine* e, const uint8_t* terms_blob, const uint64_t* term_off, uint32_t n_terms, uint32_t flags) try {
    if (!e || (n_terms && (!terms_blob || !term_off))) return e ? fail(e, GFT_E_INVALID, "null argument") : GFT_E_INVALID;
    GFT_LOCK(e);
    if (!e->peers.empty() && !e->in_multi) return multi_build(e, terms_blob, term_off, n_terms, flags);
    if (int rc = check_ready(e, kNeedDevice)) return rc;
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
    if (int rc = check_ready(e, kNeedBuilt)) return rc;
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
    int rc = read_tables(blob, len, set, flags, e->err);
    if (rc) return rc;          // the handle is untouched: the dictionary installed before, if any, still is
    if ((rc = check_ready(e, kNeedDevice))) return rc;
    return install_tables(e, std::move(set), flags);
} GFT_CATCH((e ? &e->err : nullptr))

int gft_set_programs(gft_engine* e, const uint32_t* prog_words, const uint64_t* prog_off, uint32_t n_exprs,
                     uint32_t n_extra) try {
    if (!e || (n_exprs && (!prog_words || !prog_off))) return e ? fail(e, GFT_E_INVALID, "null argument") : GFT_E_INVALID;
    GFT_LOCK(e);
    e->have_labels = false;     // (labels belong to a set of programs: gft_set_expr_labels)
    e->h_labels.clear();
    if (!e->peers.empty() && !e->in_multi) return multi_set_programs(e, prog_words, prog_off, n_exprs, n_extra);
    if (int rc = check_ready(e, kNeedDevice | kNeedBuilt)) return rc;
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
    e->d_spans.wit_ready = false;
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

int gft_set_expr_labels(gft_engine* e, const uint32_t* labels, uint32_t n) try {
    if (!e) return GFT_E_INVALID;
    GFT_LOCK(e);
    e->have_labels = false;
    e->h_labels.clear();
    if (!labels || !n) {
        if (labels || n) return fail(e, GFT_E_INVALID, "gft_set_expr_labels: labels and n go together (NULL, 0 clears)");
        return GFT_OK;
    }
    if (int rc = check_ready(e, kNeedPrograms)) return rc;
    if (n != e->n_exprs) return fail(e, GFT_E_INVALID, "gft_set_expr_labels: one label per expression (n != gft_n_exprs)");
    if (int rc = check_ready(e, kNeedDevice)) return rc;
    DeviceGuard g(e->device);
    SyncOnExit drained(e);
    e->h_labels.assign(labels, labels + n);
    const int rc = upload(e, e->d_labels, e->h_labels, "label upload");
    if (rc) { e->h_labels.clear(); return rc; }
    e->have_labels = true;
    return GFT_OK;
} GFT_CATCH((e ? &e->err : nullptr))

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
    if (int rc = check_ready(e, kNeedDevice)) return rc;
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
