// gft_context.hpp -- context lines round the documents that matched (gft_context.hip): the launchers, and the same walk on the host
// (context_host.cpp), which is also what a finder takes when a batch's rows were completed on the host.
#pragma once
#include <stdint.h>

#include "../../include/gft.h"
#include "gft_context_piece.hpp"
#include "gft_select.hpp"

namespace gft {

// gft_context_docs_device's contract on host pointers: the mark pass, the reach, carry and decide passes tile by tile through
// gft_context_piece.hpp, the three prefix sums, the place pass and the select's copy walk.  Reads blob[doc_off[0], doc_off[n_docs])
// only.  Returns a gft_status.
int context_docs_host(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const uint32_t* bitmap, uint32_t n_cols,
                      const uint32_t* want, uint32_t mode, const uint8_t* also, uint64_t before, uint64_t after, const uint8_t* fence,
                      uint8_t* out, uint64_t cap_bytes, uint64_t* out_off, uint64_t* doc_idx, uint8_t* kind, uint64_t cap_docs,
                      uint64_t* group_off, uint64_t cap_groups, uint64_t* n_kept, uint64_t* n_hits, uint64_t* n_groups, uint64_t* total_bytes);

// select_buffers_overlap's sibling for this call: one input more (the fences), two outputs more (kind, group_off)
inline bool context_buffers_overlap(const uint8_t* text, uint64_t lo, uint64_t hi, const uint64_t* doc_off, uint64_t n_docs,
                                    const uint32_t* bitmap, uint32_t n_cols, const uint8_t* also, const uint8_t* fence, const uint8_t* out,
                                    uint64_t cap_bytes, const uint64_t* out_off, const uint64_t* doc_idx, const uint8_t* kind, uint64_t cap_docs,
                                    const uint64_t* group_off, uint64_t cap_groups) {
    const ByteRange outs[] = {{out, cap_bytes}, {out_off, out_off ? (cap_docs + 1) * 8 : 0}, {doc_idx, cap_docs * 8}, {kind, cap_docs},
                              {group_off, group_off ? (cap_groups + 1) * 8 : 0}};
    const ByteRange ins[] = {{text ? text + lo : nullptr, hi > lo ? hi - lo : 0}, {doc_off, (n_docs + 1) * 8},
                             {bitmap, n_docs * ((n_cols + 31) / 32) * 4}, {also, n_docs}, {fence, n_docs}};
    return outputs_overlap(outs, ins);
}

}  // namespace gft

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace gft {

struct ContextParams {
    const uint64_t* doc_off;   // [n_docs + 1]
    uint64_t n_docs, n_tiles, n_blocks;
    const uint32_t* sel;       // [n_docs]       k_select_mark's flag; the decide pass reuses the array for newgroup
    const uint8_t* fence;      // [n_docs] or NULL
    uint64_t before, after;
    uint64_t* word_sel;        // [n_tiles]      reach: the tile's ballot words
    uint64_t* word_fence;
    uint64_t* sum;             // [4][n_tiles]   reach: last selected, last fence (index + 1), first selected, first fence
    uint64_t* carry;           // [4][n_tiles]   carry: the same four over the tiles in front / behind
    uint64_t* part;            // [5][n_blocks]  the carry blocks' own four, then over the blocks in front / behind; their selected counts
    uint32_t* keep;            // [n_docs]       decide
    uint32_t* len;             // [n_docs]
    uint32_t* newgroup;        // [n_docs]
    const uint64_t* pos;       // [n_docs + 1]   exclusive prefix sums of len, keep, newgroup
    const uint64_t* rank;
    const uint64_t* grank;
    uint64_t* ctl;             // [kCtxCtlWords] the select's words (the flag is k_select_mark's), then hits and groups
    uint64_t* c_off;           // [m + 1]        place -> the select's copy pass
    uint64_t* c_src;           // [m]
    uint64_t m, total, groups;
    uint64_t* out_off;         // [cap_docs + 1] or NULL
    uint64_t* doc_idx;         // [cap_docs]
    uint8_t* kind;             // [cap_docs]
    uint64_t cap_docs;
    uint64_t* group_off;       // [cap_groups + 1] or NULL
    uint64_t cap_groups;
};

hipError_t launch_context_reach(const ContextParams& P, unsigned n_cus, hipStream_t st);
hipError_t launch_context_carry(const ContextParams& P, unsigned n_cus, hipStream_t st);
hipError_t launch_context_decide(const ContextParams& P, unsigned n_cus, hipStream_t st);
hipError_t launch_context_pack(const ContextParams& P, hipStream_t st);
hipError_t launch_context_place(const ContextParams& P, hipStream_t st);

}  // namespace gft
#endif
