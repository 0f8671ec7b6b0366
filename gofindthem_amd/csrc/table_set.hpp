// table_set.hpp -- everything the library keeps about a dictionary on the host, and what it decides from it: the three
// table compilers as one step, the table blob of gft_export_tables / gft_import_tables (writer, reader, validation), the
// choice of the scan kernel with its LDS plan and the tables derived for scan5.  Host arithmetic only: no
// device, no handle -- gft_build / gft_import_tables upload what comes out, gft_debug_tables runs it on the CPU.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "ac_tables.hpp"
#include "gft_kernels.hpp"
#include "scan2_tables.hpp"
#include "scan3_tables.hpp"

namespace gft {

struct TableSet {
    AcTables tab;          // the automaton: the DFA kernel's tables, and the term list
    Scan2Tables s2;        // scan2's tables: what scan2, scan4 and scan5 run on
    Scan3Tables s3;        // scan3's: the stride-2 suffix-window kernel, any alphabet
};

// terms may contain duplicates and the empty string (build_ac_tables)
void compile_tables(std::vector<std::string> terms, TableSet& out);

// ---- the set as one blob (BuildEngine for a large dictionary is paid once) -------------------------
constexpr uint32_t kTablesVersion = 9;           // bump when a table layout or a hash function changes
void write_tables(const TableSet& ts, uint32_t flags, std::vector<uint8_t>& out);
// GFT_OK, or the status of the refusal with its text in `err` -- `out` and `flags` are then untouched.  A blob that passes
// the checksum may still be stale or crafted: every index a kernel follows is checked against the table it indexes.
int read_tables(const uint8_t* blob, uint64_t len, TableSet& out, uint32_t& flags, std::string& err);

// ---- the scan kernel of a set ----------------------------------------------------------------------------------------
// The kernel that scans the text: the two-tier DFA kernel (gft_kernels.hip: an independent algorithm, the cross-check) or
// one of the suffix-window kernels.  Those count the slabs of the match pool that their waves take, the DFA kernel counts
// its matches.
enum class ScanKernel { dfa, scan2, scan3, scan4, scan5 };
constexpr const char* kScanKernelName[] = {"dfa", "scan2", "scan3", "scan4", "scan5"};
constexpr bool counts_slabs(ScanKernel k) { return k != ScanKernel::dfa; }     // ... and leaves a unit's matches unsorted
constexpr bool on_scan2_tables(ScanKernel k) { return k == ScanKernel::scan2 || k == ScanKernel::scan4 || k == ScanKernel::scan5; }

// GFT_SCAN_KERNEL: the kernel the caller asks for ("auto", empty and null: none)
enum class Forced { none, dfa, scan2, scan3, scan4, scan5, unknown };
Forced parse_forced(const char* name);

// what the environment says about the choice; the library reads it in one place, scan_options() of gft_api.cpp
struct ScanOptions {
    Forced forced = Forced::none;
    uint32_t scan5_bloom_kb = 32;          // GFT_SCAN5_BLOOM_KB: the Bloom level's size in LDS (0: none; a power of two up to 64)
    uint32_t scan5_large = 1;              // GFT_SCAN5_LARGE=0: dictionaries over more than 32 byte classes stay on scan3
    uint32_t scan5_fifo = 0;               // GFT_SCAN5_FIFO: entries of a wave's match fifo (0: 256; timing study)
    uint32_t scan5_groups = 0;             // GFT_SCAN5_GROUPS: forced number of filter groups (tests)
};

// the chosen kernel and what its LDS plan says (the fields of the kernels that were not chosen mean nothing)
struct ScanPlan {
    ScanKernel kernel = ScanKernel::dfa;
    uint32_t scan_waves = 0;               // its waves per workgroup (dfa: 0, it owns no slabs)
    uint32_t n_lds_states = 0;             // dfa: rows of the transition table that fit LDS
    uint32_t scan2_cand_cap = 0;           // scan2_plan
    uint32_t scan3_cand_cap = 0;           // scan3_plan
    uint32_t scan4_fifo[2] = {0, 0};       // scan4_plan: fifo entries without / with positions
    Scan5Plan s5plan{0, 0, 0, 0};          // scan5_plan
    uint32_t s5_bloom_lg = 0;              // the Bloom level in front of a global fingerprint table: 2^lg bits; 0: none
    uint32_t s5_term_bits = 0, s5_pos_bias = 0;   // the shape of a fifo entry: term id and relative position in 32 bits
    bool s5_short_groups = false;          // scan5's short terms come from scan3's tables (> 32 byte classes)
};

// The scan kernel for a set on a device with `lds_max` bytes of LDS per workgroup (the table of DESIGN.md 4.7).  scan5 is
// the default wherever it applies, scan3 (any alphabet) everywhere else; scan2 / scan4 (`extra_kernels`: the library
// carries them) and the DFA kernel are cross-checks that `opt.forced` asks for.  GFT_OK, or GFT_E_UNSUPPORTED with the
// text in `err` (a keyword or an automaton beyond the limits, LDS too small, a kernel that is not built in) -- `out` is
// then untouched.
int plan_scan(const TableSet& ts, const ScanOptions& opt, size_t lds_max, bool extra_kernels, ScanPlan& out, std::string& err);

// what scan5 reads on top of the set (plan.kernel == scan5): the filter over plan.s5plan.G merged classes, and the Bloom
// level's words (empty when plan.s5_bloom_lg == 0)
void derive_scan5(const TableSet& ts, const ScanPlan& plan, Scan5Tables& s5, std::vector<uint32_t>& bloom);

}  // namespace gft
