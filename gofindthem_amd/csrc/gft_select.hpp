// gft_select.hpp -- the documents that matched, gathered into one blob (gft_select.hip): the launchers, and the same walk on the
// host (select_host.cpp), which is also what a finder selects with when a batch's rows were completed on the host.
#pragma once
#include <stdint.h>

#include "../../include/gft.h"
#include "gft_bitrows.hpp"
#include "gft_overlap.hpp"
#include "gft_select_piece.hpp"

namespace gft {

// gft_select_docs_device's contract on host pointers: the mark pass, the two prefix sums, the place pass and the copy pass, tile
// by tile through gft_select_piece.hpp.  Reads blob[doc_off[0], doc_off[n_docs]) only.  Returns a gft_status.
int select_docs_host(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const uint32_t* bitmap, uint32_t n_cols,
                     const uint32_t* want, uint32_t mode, const uint8_t* also, uint8_t* out, uint64_t cap_bytes, uint64_t* out_off,
                     uint64_t* doc_idx, uint64_t cap_docs, uint64_t* n_selected, uint64_t* total_bytes);

// The mark pass of k_select_mark over every document: sel[d], and len[d] where len is asked for; wm: `want` as select_want_words
// leaves it.  False when offsets descend or a document has 4 GiB or more.
bool select_mark_host(const uint64_t* doc_off, uint64_t n_docs, const uint32_t* bitmap, uint32_t W, const uint32_t* wm, uint32_t mode,
                      const uint8_t* also, uint32_t* sel, uint32_t* len);

// the copy pass alone, every tile of G: the compact arrays c_off [m + 1] / c_src [m] in whatever order their entries come
void select_copy_host(const uint8_t* text, const uint64_t* c_off, const uint64_t* c_src, uint64_t m, const SelGeom& G, uint8_t* out);

// `want` as the mark pass reads it: W = ceil(n_cols / 32) words, NULL = every column, the bits at and above n_cols cleared
inline void select_want_words(const uint32_t* want, uint32_t n_cols, uint32_t* dst) {
    const uint32_t W = (n_cols + 31) / 32;
    for (uint32_t j = 0; j < W; j++) dst[j] = want ? want[j] : 0xFFFFFFFFu;
    if (W && (n_cols & 31)) dst[W - 1] &= (1u << (n_cols & 31)) - 1;
}

// an output of the call overlaps one of its inputs (the text is [lo, hi) of the blob), or another output
inline bool select_buffers_overlap(const uint8_t* text, uint64_t lo, uint64_t hi, const uint64_t* doc_off, uint64_t n_docs,
                                   const uint32_t* bitmap, uint32_t n_cols, const uint8_t* also, const uint8_t* out, uint64_t cap_bytes,
                                   const uint64_t* out_off, const uint64_t* doc_idx, uint64_t cap_docs) {
    const ByteRange outs[] = {{out, cap_bytes}, {out_off, out_off ? (cap_docs + 1) * 8 : 0}, {doc_idx, cap_docs * 8}};
    const ByteRange ins[] = {{text ? text + lo : nullptr, hi > lo ? hi - lo : 0}, {doc_off, (n_docs + 1) * 8},
                             {bitmap, n_docs * ((n_cols + 31) / 32) * 4}, {also, n_docs}};
    return outputs_overlap(outs, ins);
}

}  // namespace gft

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace gft {

struct SelectParams {
    const uint8_t* text;
    const uint64_t* doc_off;   // [n_docs + 1]
    uint64_t n_docs;
    const uint32_t* bitmap;    // [n_docs][W]
    uint32_t W, lg;            // words per row; W <= 64: a row is a segment of 1 << lg lanes
    uint32_t mode;
    const uint32_t* want;      // [W]            the engine's copy, cut to n_cols
    const uint8_t* also;       // [n_docs] or NULL
    uint32_t* len;             // [n_docs]       mark: the document's length if selected, else 0
    uint32_t* sel;             // [n_docs]       mark: 0 / 1
    const uint64_t* pos;       // [n_docs + 1]   exclusive prefix sum of len
    const uint64_t* rank;      // [n_docs + 1]   ... of sel
    uint64_t* ctl;             // [kSelCtlWords] (the context call: [kCtxCtlWords], its own block)
    uint64_t* c_off;           // [m + 1]        place -> copy
    uint64_t* c_src;           // [m]
    uint64_t m, total;
    uint8_t* out;
    uint64_t* out_off;         // [cap_docs + 1] or NULL
    uint64_t* doc_idx;         // [cap_docs]
    uint64_t cap_docs;
    SelGeom G;
};

hipError_t launch_select_mark(const SelectParams& P, unsigned n_cus, hipStream_t st);
hipError_t launch_select_pack(const SelectParams& P, hipStream_t st);
hipError_t launch_select_place(const SelectParams& P, hipStream_t st);
hipError_t launch_select_copy(const SelectParams& P, hipStream_t st);

}  // namespace gft
#endif
