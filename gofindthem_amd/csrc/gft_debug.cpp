// gft_debug.cpp -- the gft_debug_* hooks of include/gft.h: host restatements and pure planners that the tests and tools
// call without a device (gft_debug_learned_unit, gft_debug_last_unit_route, gft_debug_last_fold_bits and
// gft_debug_last_solve_pf alone read a handle).
#include "gft_engine.hpp"

#include <unordered_set>

#include "host_solve.hpp"

using namespace gft;
using namespace gft::api;

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

int gft_debug_last_unit_route(const gft_engine* e, const char** name) {
    if (!e || !name) return GFT_E_INVALID;
    *name = e->last_unit_route;
    return GFT_OK;
}

int gft_debug_last_fold_bits(const gft_engine* e, uint32_t* bits) {
    if (!e || !bits) return GFT_E_INVALID;
    *bits = e->reported.nonascii_bits;
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

int gft_debug_pool_entries(const gft_engine* e, uint64_t* entries) {
    if (!e || !entries) return GFT_E_INVALID;
    *entries = e->pool.total;
    return GFT_OK;
}

int gft_debug_last_solve_pf(const gft_engine* e, uint32_t* pf_terms, uint32_t* unit_entries) {
    if (!e || !pf_terms) return GFT_E_INVALID;
    *pf_terms = e->last_pf_terms;
    if (unit_entries) *unit_entries = e->learned.unit_entries;
    return GFT_OK;
}

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

}  // extern "C"
