// batch_verdict.hpp -- what a batch reports back, as values: the control block the kernels of a batch write and the host
// reads once, the verdict a scan established, what a scan launch knew, the judgement on a launch that ran without knowing
// its sizes, and what batches teach the next ones.  Host arithmetic only: no device, no handle -- gft_pipeline.cpp reads the
// block back and applies the judgement, gft_debug_judge_batch / gft_debug_learn run the same functions on the CPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "table_set.hpp"

namespace gft {

// ---- the control block (device, 64 bytes; one memset per batch, one read-back per synchronisation) ----------------------
//   word 0   [0]  u32  bad-offsets flag (k_unit_count: non-zero; k_units_single: raised to the batch's epoch)
//   word 1   [8]  u64  pool cursor (suffix-window kernels: entries taken behind the slabs the waves own; DFA kernel: matches)
//   word 2   [16] u64  exact match count (suffix-window kernels)
//   word 3   [24] u32  non-ASCII bits of a folded scan: 1 = bytes >= 0x80 seen, not judged; 2 = judged unsafe (k_fold_safe too)
//            [28] u32  k_units_single: raised to the batch's epoch when a document is longer than one unit
//   word 4   [32] u64  n_units    \.
//   word 5   [40] u64  text_lo     > k_pack_ctl / k_units_single: first and last text offset of the batch
//   word 6   [48] u64  text_hi    /
constexpr size_t kCtlBytes = 64, kCtlWords = 7;            // allocated; the words of a full read-back
constexpr size_t kCtlBad = 0, kCtlCursor = 8, kCtlTotal = 16, kCtlNonascii = 24, kCtlUnits = 32;
constexpr size_t kCtlBatchClear = 32;                      // memset in front of a batch: [0, 32) -- flag, cursor, count, word 3
constexpr size_t kCtlRetryClear = 16;                      // ... of another attempt of its scan: [kCtlCursor, +16) -- cursor, count
constexpr size_t kCtlScanRead = 24;                        // read-back behind a scan alone: [kCtlCursor, +24) -- words 1 .. 3

struct CtlBlock {
    uint32_t bad = 0;                      // word 0
    uint64_t cursor = 0, total = 0;        // as the kernels left them: without the slabs a launch owned from the start
    uint32_t nonascii_bits = 0;
    uint32_t miss_epoch = 0;               // the high half of word 3
    uint64_t n_units = 0, text_lo = 0, text_hi = 0;
};
CtlBlock decode_ctl(const uint64_t words[kCtlWords]);

// What one batch's scan established -- the only carrier of these values between the stages of a batch and to its caller
struct BatchVerdict {
    bool nonascii = false;                 // a GFT_FOLD_ASCII scan over text that ASCII folding does not lower-case the way
                                           // strings.ToLower does (gft_last_nonascii)
    uint32_t nonascii_bits = 0;            // what the scan kernels said (CtlBlock); refine_nonascii turns them into `nonascii`
    uint64_t text_lo = 0, text_hi = 0;     // text range of the scan
    uint64_t n_units = 0, total = 0;       // work units and matches
};

// What a scan launch knew.  A deferred launch (scan_pipeline) ran without a read-back of the unit count or the pool need:
// its caller judges it against these numbers after its last kernel -- the engine's own may have changed by then, for a
// younger batch, but the kernels of this launch wrote nothing beyond unit_cap and pool_cap.
struct ScanLaunch {
    bool deferred = false;
    bool single = false;                   // the unit table came from k_units_single ...
    uint32_t epoch = 0;                    // ... which raises the batch's control-block flags to this number
    bool ordered = false;                  // every unit went through scan2's per-lane staging path (GFT_SCAN_ORDERED)
    uint64_t n_docs = 0, unit_cap = 0, pool_cap = 0;
    uint64_t static_slabs = 0;             // pool entries that the waves of the grid owned from the start (the cursor counts behind them)
};

// a k_units_single launch met a document of more than one unit: the batch goes the general way
inline bool single_miss(const CtlBlock& c, const ScanLaunch& L) { return L.single && c.miss_epoch == L.epoch; }

// The verdict on a deferred launch from the read-back of the control block that its caller made after the batch's last
// kernel -- the batch's only host synchronisation.  again_*: the batch is run once more, this time with the sizes known
// (again_general: a k_units_single miss, or more units than the table held; again_grow: the scan needed pool_need entries
// of match pool, more than the launch had -- whatever the pool holds by now, the launch wrote nothing beyond its own).
struct Judgement {
    enum Kind { accept, again_general, again_grow, invalid } kind = accept;
    uint64_t pool_need = 0;                // again_grow only
    const char* err = "";                  // invalid only
    BatchVerdict verdict;
};
Judgement judge_deferred(const CtlBlock& c, const ScanLaunch& L);

// ---- what the batches teach the next ones ---------------------------------------------------------------------------------
struct Learned {
    // batches in a row that were one unit per document (k_units_single serves the next one from 2 on; a batch that took
    // that path and held a longer document after all sets it well below zero, so that a corpus whose batches alternate does
    // not pay for the miss every other time)
    int single_streak = 0;
    uint32_t unit_max = kScan2UnitMax;     // bytes per work unit of the kernels on scan2's tables: follows the match density
    double scan4_density = 0.06;           // matches per text byte: scan4 sizes a unit's region of the match pool from it
    uint32_t unit_entries = 0;             // mean pool entries per unit of the last completed batch, rounded up (0: none yet, or
                                           // none matched): the solver's prefetch depth follows it (solve_plan.hpp)
};
constexpr int kSingleMissStreak = -8;
inline void count_streak(Learned& s, uint64_t n_units, uint64_t n_docs) {
    s.single_streak = n_units == n_docs ? s.single_streak + 1 : std::min(s.single_streak, 0);
}
// a completed batch of `total` matches over [text_lo, text_hi); fifo_cap: the entries of a wave's LDS match fifo
void learn(Learned& s, ScanKernel kernel, uint32_t fifo_cap, bool ordered, uint64_t total, uint64_t text_lo, uint64_t text_hi);

}  // namespace gft
