// gft_stats.hpp -- term statistics of a match or span list and column counts of a hit bitmap (gft_stats.hip): the launchers, and
// the same walks on the host (stats_host.cpp).
#pragma once
#include <stdint.h>

#include "../../include/gft.h"
#include "gft_overlap.hpp"
#include "gft_stats_piece.hpp"

namespace gft {

// gft_term_stats_device's contract on host pointers: the check, then the count pass workgroup by workgroup, step by step and lane
// by lane through gft_stats_piece.hpp (the set, the bitset and the cache included).  Returns a gft_status; a refusal writes nothing.
int term_stats_host(const uint64_t* off, const uint32_t* term, uint64_t n_docs, uint32_t n_terms, uint32_t flags, uint64_t doc_base,
                    uint64_t* occ, uint64_t* docs, uint64_t* first);
// gft_count_columns_device's contract on host pointers, workgroup by workgroup
int count_columns_host(const uint32_t* bitmap, uint64_t n_rows, uint32_t n_cols, const uint64_t* row_idx, uint32_t flags, uint64_t* count);

// an output of the term statistics overlaps an input (the entries are [e0, e0 + n) of term) or another output
inline bool stats_buffers_overlap(const uint64_t* off, uint64_t n_docs, const uint32_t* term, uint64_t e0, uint64_t n, uint32_t n_terms,
                                  const uint64_t* occ, const uint64_t* docs, const uint64_t* first) {
    const uint64_t out_n = (uint64_t)n_terms * 8;
    const ByteRange outs[] = {{occ, out_n}, {docs, out_n}, {first, out_n}};
    const ByteRange ins[] = {{off, (n_docs + 1) * 8}, {term ? term + e0 : nullptr, n * 4}};
    return outputs_overlap(outs, ins);
}
// the counts overlap the bitmap (its first n_rows rows; with row_idx the rows' extent is the caller's) or the row indices
inline bool columns_buffers_overlap(const uint32_t* bitmap, uint64_t n_rows, uint32_t n_cols, const uint64_t* row_idx, const uint64_t* count) {
    const ByteRange outs[] = {{count, (uint64_t)n_cols * 8}};
    const ByteRange ins[] = {{bitmap, (row_idx ? 0 : n_rows) * stats_col_words(n_cols) * 4}, {row_idx, n_rows * 8}};
    return outputs_overlap(outs, ins);
}

}  // namespace gft

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace gft {

// Work buffers: 16 bytes of flag words; with n_terms > kStatsBitsetLdsTerms a bitset row of ceil(n_terms / 32) * 4 bytes per
// workgroup of the count pass.  Nothing per entry.
struct StatsParams {
    const uint64_t* off;           // [n_docs + 1]
    const uint32_t* term;
    uint64_t n_docs, e0, n;        // the entries are [e0, e0 + n)
    uint32_t n_terms, accumulate;
    uint64_t doc_base;
    uint64_t* occ;                 // each NULL or [n_terms]
    uint64_t* docs;
    uint64_t* first;
    uint64_t* ctl;                 // [kStatsCtlWords]
    uint32_t* rows;                // the workgroups' bitset rows (NULL: the bitset is in LDS)
    uint32_t grid;                 // workgroups of the count pass
};

struct ColumnParams {
    const uint32_t* bitmap;
    const uint64_t* row_idx;       // NULL: row r is row r
    uint64_t n_rows;
    uint32_t n_cols;
    uint64_t* count;
};

hipError_t launch_stats_check(const StatsParams& P, unsigned n_cus, hipStream_t st);
hipError_t launch_stats_init(const StatsParams& P, hipStream_t st);
hipError_t launch_stats_count(const StatsParams& P, hipStream_t st);
// workgroups of the count pass that are resident at a time on a device of n_cus compute units
uint32_t stats_resident(unsigned n_cus);
hipError_t launch_count_columns(const ColumnParams& P, hipStream_t st);

}  // namespace gft
#endif
