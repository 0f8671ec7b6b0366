// scan5_plan_check.cpp -- the host side of the k_scan5 launch (the table build and the LDS plan: build_ac_tables,
// build_scan2_tables, scan5_plan of gft_scan5.hip, build_scan5_tables) under the address and undefined-behaviour sanitizers: a
// stand-alone program, CPU only (no HIP call is made, no device is needed).
//
//   C=gofindthem_amd/csrc; F="--offload-arch=gfx950 -std=c++17 -O1 -g"
//   XS="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined"      # (host code only)
//   hipcc $F $XS -c $C/gft_scan5.hip -o build/spc_scan5.o
//   hipcc -x hip $F $XS -I. -c tools/scan5_plan_check.cpp -o build/spc_main.o
//   hipcc -x hip $F $XS -c $C/ac_tables.cpp -o build/spc_ac.o
//   hipcc -x hip $F $XS -c $C/scan2_tables.cpp -o build/spc_s2.o
//   hipcc build/spc_main.o build/spc_ac.o build/spc_s2.o build/spc_scan5.o -fsanitize=address,undefined -o build/scan5_plan_check
//   build/scan5_plan_check
//
// Dictionaries: two byte classes up to the whole byte range, with and without terms shorter than the window, a few hundred terms
// that share suffixes.  For each: every LDS budget from too small to the device's, both fifo sizes the engine uses; a plan that
// fits is checked against the budget by the formulas of the launch and its filter is built at the plan's G.
// Exit code 0: every plan fits its budget and every filter has G^3 entries.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "gofindthem_amd/csrc/ac_tables.hpp"
#include "gofindthem_amd/csrc/gft_kernels.hpp"
#include "gofindthem_amd/csrc/scan2_tables.hpp"

using namespace gft;

static std::vector<std::string> dictionary(std::mt19937& rng, const std::string& alphabet, int n, int min_len, int max_len) {
    std::vector<std::string> t;
    for (int i = 0; i < n; i++) {
        const int L = min_len + (int)(rng() % (unsigned)(max_len - min_len + 1));
        std::string s;
        for (int j = 0; j < L; j++) s.push_back(alphabet[rng() % alphabet.size()]);
        if (i % 7 == 0) s += "wxyz";                     // shared suffix: buckets with several entries
        t.push_back(s);
    }
    return t;
}

int main() {
    std::mt19937 rng(12345);
    std::string all;
    for (int b = 1; b < 256; b++) all.push_back((char)b);
    struct Case { std::string alphabet; int n, lo, hi; };
    const Case cases[] = {{"ab", 12, 1, 9},   {"abcdefgh", 300, 1, 12}, {"abcdefghijklmnopqrstuvwxyz", 2000, 1, 30},
                          {"abcde", 200, 4, 12}, {"abcdefghijklmnopqrstuvwxyz0123456789 .-_", 400, 1, 11}, {all, 500, 1, 40}};
    int plans = 0, fits = 0;
    for (const Case& c : cases) {
        AcTables ac;
        build_ac_tables(dictionary(rng, c.alphabet, c.n, c.lo, c.hi), ac);
        Scan2Tables s2;
        build_scan2_tables(ac, s2);
        if (!s2.long_ok) { std::printf("alphabet of %zu bytes: no suffix-window tables (%s)\n", c.alphabet.size(), s2.why_not); continue; }
        const uint32_t short_bytes = s2.short_direct ? (uint32_t)s2.short3.size() : 0u;
        const uint32_t rec_words = (uint32_t)std::min<size_t>(s2.shorts_packed.size(), 255 * 3);
        const uint32_t in_lds = s2.fpt_lg == 0 ? kScan2FptSize : 0u;
        for (size_t lds_max : {(size_t)8 << 10, (size_t)32 << 10, (size_t)64 << 10, (size_t)100 << 10, ((size_t)160 << 10) - 512}) {
            for (uint32_t fifo : {64u, (uint32_t)kScan2FifoCap}) {
                Scan5Plan p{0, 0, 0, 0};
                plans++;
                if (!scan5_plan(s2.kp, short_bytes, rec_words, in_lds, lds_max, fifo, &p)) continue;
                fits++;
                const size_t fixed = ((768 + (size_t)p.dual_entries * 8 + short_bytes + in_lds + (size_t)rec_words * 4 + 15) & ~(size_t)15) + 16;
                const size_t wave = (size_t)p.fifo_cap * 4 + kScan5SurvX * 4 + kScan5SeenWords * 4 + (((size_t)p.cand_cap * 2 + 15) & ~(size_t)15);
                if (fixed + kScan5Waves * wave > lds_max || p.G < 2 || p.G > kScan5MaxGroups || p.G > s2.kp || p.dual_entries != p.G * p.G * p.G ||
                    p.cand_cap < kScan5CandCapMin || p.fifo_cap != fifo) {
                    std::printf("bad plan: G %u, list %u, fifo %u for %zu bytes\n", p.G, p.cand_cap, p.fifo_cap, lds_max);
                    return 1;
                }
                Scan5Tables s5;
                build_scan5_tables(ac, s2, p.G, s5);
                if (s5.G != p.G || s5.filter.size() != p.dual_entries || s5.pad_group >= s5.G) { std::printf("bad filter at G %u\n", p.G); return 1; }
                for (int b = 0; b < 256; b++)
                    if (s5.grp[b] >= s5.G || s5.grp_fold[b] >= s5.G) { std::printf("group of byte %d out of range\n", b); return 1; }
            }
        }
    }
    std::printf("scan5_plan_check: %d plans asked, %d fit, all inside their budget\n", plans, fits);
    return fits ? 0 : 1;
}
