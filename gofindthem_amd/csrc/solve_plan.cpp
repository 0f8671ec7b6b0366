// solve_plan.cpp -- see solve_plan.hpp
#include "solve_plan.hpp"

#include <algorithm>

#include "gft_guard.hpp"

namespace gft {

// (device-side counterpart: the pointer arithmetic at the top of k_solve_groups, gft_solve.hip)
size_t solve_lds_bytes(uint32_t n_slots, uint32_t tile_words, uint32_t group_docs, bool p_in_lds, uint32_t prog_words,
                       uint32_t n_exprs, bool prog_in_lds) {
    return (p_in_lds ? (((size_t)n_slots * (group_docs / 8) + 15) & ~(size_t)15) : 0) + (size_t)64 * (tile_words | 1u) * 4 +
           (size_t)tile_words * 32 * 8 + (prog_in_lds ? ((size_t)prog_words + 2 * (size_t)n_exprs + 1) * 4 : 0);
}

// LDS that a choice leaves free (bytes): what the presence matrix and the programs must leave of lds_max to be placed
// there, and what a workgroup is counted to need beyond its dynamic LDS when the workgroups per CU are worked out.  Three
// constants as they were measured with, not one.
constexpr size_t kSlackPresence = 1024, kSlackPrograms = 1024, kSlackPerCu = 512;

SolvePlan plan_solve(const SolveShape& s, size_t lds_max, unsigned n_cus, uint64_t n_docs, const SolveOptions& opt) {
    SolvePlan p;
    p.tile_words = std::min<uint32_t>(kSolveTileWords, (s.n_exprs + 31) / 32);
    const bool wide = s.wide_pairs != 0;
    p.wide_cap = (s.wide_pairs + 63u) & ~63u;
    p.rare = wide ? 2u : s.has_rare ? 1u : 0u;
    // Presence matrix in LDS next to the output tile: G documents per group = G / 8 bytes per slot, the widest G of
    // 64 / 32 / 16 / 8 that fits (opt.forced_group: that width or none); beyond that in HBM (served by L2), where G = 64
    p.group_docs = 64;
    p.p_in_lds = false;
    for (uint32_t G : {64u, 32u, 16u, 8u}) {
        if (opt.forced_group >= 0 && (uint32_t)opt.forced_group != G) continue;
        if (solve_lds_bytes(s.n_slots, p.tile_words, G, true, 0, 0, false) + kSlackPresence <= lds_max) { p.group_docs = G; p.p_in_lds = true; break; }
    }
    // ... and the fused programs too, if there is room left (the interpreter fetches them word after word).  A set with a
    // wide INORD group never: the kernels that can call the wide paths read their programs from L2
    p.prog_in_lds = !wide && opt.prog_lds &&
                    solve_lds_bytes(s.n_slots, p.tile_words, p.group_docs, p.p_in_lds, s.fprog_words, s.n_exprs, true) + kSlackPrograms <= lds_max;
    // timing studies: the benchmark's shape (presence matrix and programs in LDS, 64 documents per group) and the shape of
    // a 100 000-term dictionary (8 documents per group, programs in L2) only; any other shape runs its production kernel
    p.dbg_variant = opt.dbg && !wide && p.p_in_lds && ((p.group_docs == 64 && p.prog_in_lds) || (p.group_docs == 8 && !p.prog_in_lds));
    // the build's prefetch depth (kPfShallowEntries): only the kernels without a NOT / INORD word pipeline and have two
    const bool shallow = opt.forced_pf ? opt.forced_pf == 6 : s.unit_entries > 0 && s.unit_entries <= kPfShallowEntries;
    p.pf_terms = p.rare == 0 && shallow ? 6u : 12u;
    p.lds_bytes = solve_lds_bytes(s.n_slots, p.tile_words, p.group_docs, p.p_in_lds, s.fprog_words, s.n_exprs, p.prog_in_lds);
    const uint64_t n_groups = (n_docs + p.group_docs - 1) / p.group_docs;
    p.per_cu = (unsigned)std::max<size_t>(1, std::min<size_t>(8, lds_max / (p.lds_bytes + kSlackPerCu)));
    p.grid = (unsigned)std::min<uint64_t>(n_groups, (uint64_t)n_cus * p.per_cu);
    return p;
}

bool solve_kernel_exists(const SolvePlan& p) {
#define X(P_LDS, PROG_LDS, G, RARE, DBG, PF) if (solve_kernel_is(p, P_LDS, PROG_LDS, G, RARE, DBG, PF)) return true;
    GFT_SOLVE_KERNELS(X)
#undef X
    return false;
}

}  // namespace gft

// ---- test hooks (include/gft.h): the functions above and nothing else --------------------------------------------------------
// plan[0 .. 10] as gft_debug_plan_solve documents them, plan[11] = pf_terms
extern "C" int gft_debug_plan_solve_pf(uint32_t n_slots, uint32_t n_exprs, uint32_t fprog_words, int has_rare, uint32_t wide_pairs,
                                       uint32_t unit_entries, uint64_t lds_max, uint32_t n_cus, uint64_t n_docs, int forced_group,
                                       int prog_lds, uint32_t dbg, uint32_t forced_pf, uint64_t* plan) try {
    if (!plan || (forced_pf != 0 && forced_pf != 6 && forced_pf != 12)) return GFT_E_INVALID;
    gft::SolveShape s;
    s.n_slots = n_slots; s.n_exprs = n_exprs; s.fprog_words = fprog_words; s.has_rare = has_rare != 0; s.wide_pairs = wide_pairs;
    s.unit_entries = unit_entries;
    gft::SolveOptions o;
    o.forced_group = forced_group; o.prog_lds = prog_lds != 0; o.dbg = dbg; o.forced_pf = forced_pf;
    const gft::SolvePlan p = gft::plan_solve(s, (size_t)lds_max, n_cus, n_docs, o);
    const uint64_t out[12] = {p.group_docs, p.p_in_lds, p.prog_in_lds, p.rare, p.dbg_variant, p.tile_words, p.wide_cap, p.lds_bytes,
                              p.per_cu, p.grid, gft::solve_kernel_exists(p), p.pf_terms};
    std::copy(out, out + 12, plan);
    return GFT_OK;
} GFT_CATCH(nullptr)

extern "C" int gft_debug_plan_solve(uint32_t n_slots, uint32_t n_exprs, uint32_t fprog_words, int has_rare, uint32_t wide_pairs,
                                    uint64_t lds_max, uint32_t n_cus, uint64_t n_docs, int forced_group, int prog_lds, uint32_t dbg,
                                    uint64_t* plan) try {
    if (!plan) return GFT_E_INVALID;
    uint64_t out[12];
    const int rc = gft_debug_plan_solve_pf(n_slots, n_exprs, fprog_words, has_rare, wide_pairs, 0, lds_max, n_cus, n_docs, forced_group,
                                           prog_lds, dbg, 0, out);
    if (rc == GFT_OK) std::copy(out, out + 11, plan);
    return rc;
} GFT_CATCH(nullptr)
