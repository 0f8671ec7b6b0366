// solve_plan.hpp -- which solver kernel a program set runs, and with what: the presence matrix's place and width, the
// programs' place, the kernel variant, the LDS need and the grid, decided by ONE function from a few numbers.  Host
// arithmetic only: no device, no handle, no environment -- solve_pipeline (gft_pipeline.cpp) sizes its buffers from the plan and
// hands it to launch_solve (gft_solve.hip), which looks the kernel up and decides nothing; gft_debug_plan_solve runs the
// same function on the CPU.
#pragma once
#include <cstddef>
#include <cstdint>

namespace gft {

constexpr uint32_t kSolveTileWords = 64;         // bitmap words (x32 expressions) evaluated per LDS output tile

// what the plan depends on of a program set and its dictionary
struct SolveShape {
    uint32_t n_slots = 0;          // rows of the presence matrix: terms + caller-supplied slots + 1
    uint32_t n_exprs = 0;
    uint32_t fprog_words = 0;      // words of the fused programs (ProgramSet)
    uint32_t has_rare = 0;         // some program holds a NOT or INORD word
    uint32_t wide_pairs = 0;       // pairs of the widest wide INORD group (0: the set has none)
    uint32_t unit_entries = 0;     // mean pool entries per unit of the engine's last completed batch, rounded up (0: unknown)
};

// what the environment says; the library reads it in one place, refresh_options() of gft_api.cpp
struct SolveOptions {
    int forced_group = -1;         // GFT_SOLVE_GROUP_DOCS: the only group width tried (-1: the widest that fits; a width that
                                   // does not fit, and 0, put the presence matrix in HBM)
    uint32_t prog_lds = 1;         // GFT_SOLVE_PROG_LDS=0: never stage the programs in LDS (tests: the far interpreter)
    uint32_t dbg = 0;              // GFT_SOLVE_DEBUG bits (timing studies)
    uint32_t forced_pf = 0;        // GFT_SOLVE_PF_TERMS=6|12: the prefetch depth of the pipelining kernels (0: by the last batch;
                                   // tests and A/B studies)
};

struct SolvePlan {
    uint32_t group_docs = 64;      // G: documents per group = bits of a presence-matrix element (64, 32, 16 or 8)
    bool p_in_lds = false;         // the presence matrix in LDS (false: in HBM, [grid][n_slots] of 8 bytes, and G == 64)
    bool prog_in_lds = false;      // the fused programs staged in LDS: the near interpreter (false: read from L2, the far one)
    uint32_t rare = 0;             // 0 no NOT / INORD word, 1 some, 2 some and a wide INORD group (then !prog_in_lds)
    bool dbg_variant = false;      // the kernel with the timing-study knock-outs and phase clocks
    uint32_t pf_terms = 12;        // slab entries per lane that the build keeps in flight: 12, or 6 for units of few entries (rare == 0)
    uint32_t tile_words = 0;       // bitmap words per output tile
    uint32_t wide_cap = 0;         // pairs per wave of the wide groups' scratch region (0: no wide group)
    size_t lds_bytes = 0;          // dynamic LDS of the launch
    unsigned per_cu = 1;           // workgroups per CU that this much LDS allows (at most 8)
    unsigned grid = 0;             // workgroups: a group each at a time, at most n_cus * per_cu
};

// The kernel's dynamic LDS: [P: n_slots elements of G / 8 bytes, padded to 16][O: 64 rows of tile_words | 1 words]
// [R: tile_words * 32 results of 8 bytes][fused programs, n_exprs + 1 offsets, n_exprs order entries].  The ONLY host-side
// statement of the layout; its device-side counterpart is the pointer arithmetic at the top of k_solve_groups (gft_solve.hip).
size_t solve_lds_bytes(uint32_t n_slots, uint32_t tile_words, uint32_t group_docs, bool p_in_lds, uint32_t prog_words,
                       uint32_t n_exprs, bool prog_in_lds);

// The build of the presence matrix prefetches pf_terms entries per lane of a 16-lane team one group ahead: 6 serve a unit of
// up to 96 entries from registers, 12 one of up to 192; a unit beyond that takes a second, dependent round of loads.  Depth 6
// is chosen when the last batch's units held at most kPfShallowEntries entries on average -- successive batches of one
// caller are alike -- and only for the kernels that pipeline (no NOT / INORD word).  Measured (MI355X, solver ms per step,
// three interleaved rounds, profiles/unit_boundary_ab_bench.txt and presence_once_solver_prefetch_depth.txt):
//   headline, 70.4 entries per unit:                 depth 12  0.362   depth 6  0.326
//   100 000 terms, 200 000 docs, ~140 per unit:      depth 12 12.59    depth 6 12.81    (stays at 12)
// Between the two nothing was measured: the threshold is the mean at which a unit's entries, which scatter around it, still
// mostly fit the 96 that depth 6 holds.
constexpr uint32_t kPfShallowEntries = 80;

// The plan for `n_docs` documents on a device of `n_cus` CUs and `lds_max` bytes of LDS per workgroup.
SolvePlan plan_solve(const SolveShape& s, size_t lds_max, unsigned n_cus, uint64_t n_docs, const SolveOptions& opt);

// The instantiations of k_solve_groups that the library carries, X(P_LDS, PROG_LDS, G, RARE, DBG, PF): the launch table of
// gft_solve.hip and solve_kernel_exists() are both this list.  PF: the prefetch depth, 6 or 12 where the kernel pipelines
// (RARE 0: GFT_SOLVE_PF2), 12 elsewhere.
//   presence matrix in LDS: every width, programs near or far, without / with NOT and INORD words
//   presence matrix in HBM: G = 64 only
//   a wide INORD group (RARE 2): programs from L2 only
//   timing studies (DBG): the benchmark's shape and a 100 000-term dictionary's, no wide group
#define GFT_SOLVE_PF2(X, P_LDS, PROG_LDS, G, DBG) X(P_LDS, PROG_LDS, G, 0, DBG, 12) X(P_LDS, PROG_LDS, G, 0, DBG, 6)
#define GFT_SOLVE_KERNELS(X)                                                                                                   \
    GFT_SOLVE_PF2(X, true, true, 64, false)  X(true, true, 64, 1, false, 12)  GFT_SOLVE_PF2(X, true, false, 64, false)  X(true, false, 64, 1, false, 12)   \
    GFT_SOLVE_PF2(X, true, true, 32, false)  X(true, true, 32, 1, false, 12)  GFT_SOLVE_PF2(X, true, false, 32, false)  X(true, false, 32, 1, false, 12)   \
    GFT_SOLVE_PF2(X, true, true, 16, false)  X(true, true, 16, 1, false, 12)  GFT_SOLVE_PF2(X, true, false, 16, false)  X(true, false, 16, 1, false, 12)   \
    GFT_SOLVE_PF2(X, true, true, 8, false)   X(true, true, 8, 1, false, 12)   GFT_SOLVE_PF2(X, true, false, 8, false)   X(true, false, 8, 1, false, 12)    \
    GFT_SOLVE_PF2(X, false, true, 64, false) X(false, true, 64, 1, false, 12) GFT_SOLVE_PF2(X, false, false, 64, false) X(false, false, 64, 1, false, 12)  \
    X(true, false, 64, 2, false, 12) X(true, false, 32, 2, false, 12) X(true, false, 16, 2, false, 12) X(true, false, 8, 2, false, 12)                     \
    X(false, false, 64, 2, false, 12)                                                                                          \
    GFT_SOLVE_PF2(X, true, true, 64, true)   X(true, true, 64, 1, true, 12)   GFT_SOLVE_PF2(X, true, false, 8, true)    X(true, false, 8, 1, true, 12)

inline bool solve_kernel_is(const SolvePlan& p, bool p_lds, bool prog_lds, uint32_t g, uint32_t rare, bool dbg, uint32_t pf) {
    return p.p_in_lds == p_lds && p.prog_in_lds == prog_lds && p.group_docs == g && p.rare == rare && p.dbg_variant == dbg && p.pf_terms == pf;
}
bool solve_kernel_exists(const SolvePlan& p);

}  // namespace gft
