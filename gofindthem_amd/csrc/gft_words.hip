// gft_words.hip -- whole-word matching: a match or span list filtered at word borders (gft_filter_word_matches_device), gfx950 /
// wave64.
//
//   (text, doc_off, list CSR off / pos / len or term, term_len, class table)  ->  out_off, out_pos, out_len, out_term
//
//   k_words_check  grid-stride: raises ctl[kWordsCtlOffs] for a list offset that descends, ctl[kWordsCtlTerms] for a term id that is
//                  no index of term_len (only when the lengths come from there), ctl[kWordsCtlRange] for an entry that leaves its
//                  document.  Every later launch returns at once when one is set: a refused call reads no text and writes nothing
//   k_words_mark   a lane an entry, grid-stride in tiles of kWordsTile: the entry's document by a binary search over the list
//                  offsets (n_docs + 1 entries, L2-resident at any batch the scan takes), its two edges, the predicate of
//                  gft_words_piece.hpp -> keep[i].  A latency-bound gather like k_span_mark: four single-byte loads round the
//                  edges decide an entry in ASCII surroundings, the decoders read up to six more bytes, each on its own and each
//                  inside the document; the class table (12.7 KB) is read through L2
//   (k_scan_* of gft_kernels.hip: keep -> rank)
//   k_words_place  a thread an index: out_off[d] = rank[off[d] - off[0]] for d <= n_docs, and the scatter of (pos, len, term) of
//                  every kept entry whose rank is below the cap
//
// Every launch reads only what an earlier launch stored; no atomics; plain vector stores.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gft_kernels.hpp"
#include "gft_words.hpp"

namespace gft {

namespace {

__device__ __forceinline__ bool refused(const WordsParams& P) {
    return (P.ctl[kWordsCtlOffs] | P.ctl[kWordsCtlTerms] | P.ctl[kWordsCtlRange]) != 0;      // (the same in every lane of the grid)
}

__global__ void __launch_bounds__(kWordsTile) k_words_check(const WordsParams P) {
    const uint64_t stride = (uint64_t)gridDim.x * kWordsTile, t0 = (uint64_t)blockIdx.x * kWordsTile + threadIdx.x;
    bool bad_off = false, bad_term = false, bad_range = false;
    for (uint64_t d = t0; d < P.n_docs; d += stride) bad_off |= P.off[d + 1] < P.off[d];
    for (uint64_t i = t0; i < P.n; i += stride) {
        const uint64_t m = P.e0 + i;
        uint32_t len;
        if (P.len) {
            len = P.len[m];
        } else {
            const uint32_t t = P.term[m];
            if (t >= P.n_terms) { bad_term = true; continue; }
            len = P.term_len[t];
        }
        const uint64_t d = words_doc_of(P.off, P.n_docs, m);
        uint32_t ok;
        const uint64_t start = words_entry_start(P.pos[m], len, P.pos_end, ok);
        if (!ok || !words_entry_ok(P.doc_off[d], P.doc_off[d + 1], start, len)) bad_range = true;
    }
    if (bad_off) P.ctl[kWordsCtlOffs] = 1;
    if (bad_term) P.ctl[kWordsCtlTerms] = 1;
    if (bad_range) P.ctl[kWordsCtlRange] = 1;
}

__global__ void __launch_bounds__(kWordsTile) k_words_mark(const WordsParams P) {
    if (refused(P)) return;
    const uint64_t stride = (uint64_t)gridDim.x * kWordsTile;
    for (uint64_t i = (uint64_t)blockIdx.x * kWordsTile + threadIdx.x; i < P.n; i += stride) {
        const uint64_t m = P.e0 + i;
        const uint32_t len = P.len ? P.len[m] : P.term_len[P.term[m]];
        const uint64_t d = words_doc_of(P.off, P.n_docs, m);
        const uint64_t a = P.doc_off[d], b = P.doc_off[d + 1];
        uint32_t ok;
        const uint64_t start = words_entry_start(P.pos[m], len, P.pos_end, ok);
        P.keep[i] = words_kept(P.table, P.text + a, b - a, start, start + len);
    }
}

__global__ void __launch_bounds__(kWordsTile) k_words_place(const WordsParams P) {
    if (refused(P)) return;
    const uint64_t i = (uint64_t)blockIdx.x * kWordsTile + threadIdx.x;
    if (P.out_off && i <= P.n_docs) P.out_off[i] = P.rank[P.off[i] - P.e0];
    if (i >= P.n || !P.keep[i]) return;
    const uint64_t r = P.rank[i];
    if (r >= P.cap) return;
    const uint64_t m = P.e0 + i;
    P.out_pos[r] = P.pos[m];
    if (P.out_len) P.out_len[r] = P.len ? P.len[m] : P.term_len[P.term[m]];
    if (P.out_term) P.out_term[r] = P.term[m];
}

uint64_t grid_stride_blocks(uint64_t work, unsigned n_cus) {
    return std::min<uint64_t>((work + kWordsTile - 1) / kWordsTile, (uint64_t)std::max(n_cus, 1u) * 8);
}

}  // namespace

hipError_t launch_words_check(const WordsParams& P, unsigned n_cus, hipStream_t st) {
    const uint64_t m = std::max(P.n, P.n_docs);
    if (!m) return hipSuccess;
    k_words_check<<<dim3((unsigned)grid_stride_blocks(m, n_cus)), dim3(kWordsTile), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_words_mark(const WordsParams& P, unsigned n_cus, hipStream_t st) {
    if (!P.n) return hipSuccess;
    k_words_mark<<<dim3((unsigned)grid_stride_blocks(P.n, n_cus)), dim3(kWordsTile), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_words_place(const WordsParams& P, hipStream_t st) {
    const uint64_t n = std::max(P.n_docs + 1, P.n);
    k_words_place<<<dim3((unsigned)((n + kWordsTile - 1) / kWordsTile)), dim3(kWordsTile), 0, st>>>(P);   // (the caller keeps this below 2^31)
    return hipGetLastError();
}

}  // namespace gft
