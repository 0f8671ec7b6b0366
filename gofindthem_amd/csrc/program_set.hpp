// program_set.hpp -- the solver's program compiler: public postfix programs (include/gft.h) -> everything the library
// keeps about an installed set.  Check, fusion (NOT pushed to the leaves, leaf operands folded into their operators, the
// deeper operand first), stand-ins for the programs beyond a device limit, the evaluation order per output tile, the
// blocks of 64 transposed for the kernel and their deal to the waves.  Host arithmetic only: no device, no handle --
// gft_set_programs uploads what comes out, gft_debug_eval_programs interprets it on the CPU.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace gft {

// what check_program learns about one program besides its validity
struct ProgramTraits {
    bool over_limit = false;                 // exceeds a limit of the device solver: always solved on the host
    uint32_t wide_pairs = 0;                 // > 0: an INORD group of more than kMaxPairs (slot, theta) pairs alive at once (or a pair
                                             // stack deeper than kMaxPairDepth) -- the device keeps such a group's pairs in a scratch
                                             // region of this many pairs per wave instead of one pair per lane
    std::vector<uint32_t> inord_slots;       // slots read inside INORD groups of more than one leaf (sorted, unique):
                                             // documents in which one of them has a non-ascending list go to the host
};

int check_program(const uint32_t* w, uint64_t len, uint32_t n_slots, uint32_t idx, ProgramTraits& traits, std::string& err);
uint32_t fuse_program(const uint32_t* w, uint64_t len, uint64_t gbase, std::vector<uint32_t>& out, std::vector<uint32_t>& groups);

struct ProgramSet {
    uint32_t n_exprs = 0, n_slots = 0;     // (slot n_slots itself is the never-present slot of the stand-ins)
    // the public postfix words: the host solver reads them, and so does the device inside INORD groups
    std::vector<uint32_t> prog;
    std::vector<uint64_t> prog_off;
    // what the solver kernel reads (gft_kernels.hpp SolveParams), none of them empty
    std::vector<uint32_t> fprog;           // fused programs as device words (fused_to_device), each a whole number of 4-word chunks
    std::vector<uint64_t> fprog_off;
    std::vector<uint32_t> groups;          // INORD group table: offset and length of a group's subtree in `prog`
    std::vector<uint32_t> order, blk_class, wave_blk;   // evaluation order, the interpreter of every block of 64, their deal to the waves
    std::vector<uint32_t> fprog_t, fblk_off;            // fused programs per sorted block of 64, transposed (read when they do not fit LDS)
    std::vector<uint32_t> wide_list;       // per expression with a wide INORD group: index, offset and length of its public words (may be empty)
    std::vector<uint32_t> fdepth;          // accumulator-stack depth of every fused program (what blk_class was made from)
    // what the HOST solves (host_solve.hpp): expressions beyond the device solver's limits, and INORD expressions in the
    // documents where one of their slots has a position list that is not ascending (a keyword and a regex with the same
    // literal: finder/finder.go:181-196)
    std::vector<uint32_t> host_only;       // expressions that are always solved on the host (over a device limit)
    std::vector<uint32_t> inord_exprs;     // expressions with a multi-leaf INORD group (candidates for irregular documents)
    std::vector<uint8_t> inord_slot;       // [n_slots + 1]: 1 = the slot is read inside such a group
    uint32_t fprog_words = 0;
    uint32_t n_inord_groups = 0;           // fused INORD ops + wide expressions: 0 = the solver never reads positions
    uint32_t n_rare_words = 0;             // fused NOT + INORD ops: 0 = the solver variant without their slow path
    uint32_t wide_pairs = 0;               // the widest INORD group the device solves through its scratch path (0: none)
    uint32_t n_wide = 0;                   // expressions with such a group: answered by the solver's second phase (wide_list)
};

// Compiles a whole set.  GFT_OK, or the status of the first refusal with its text in `err` -- `out` is then untouched.
int compile_programs(const uint32_t* prog_words, const uint64_t* prog_off, uint32_t n_exprs, uint32_t n_slots, ProgramSet& out,
                     std::string& err);
void print_program_stats(const ProgramSet& ps);

}  // namespace gft
