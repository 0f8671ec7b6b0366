// gft_spans.hip -- hit spans and redaction (gft_hit_spans_device, gft_redact_spans_device), gfx950 / wave64.
//
//   (match CSR of the scan, hit rows, row_idx, want, witness table)  ->  span_off, span_start, span_len, span_term
//
//   k_span_mark    a lane a match, grid-stride: the match's document by a binary search over match_off (n_docs + 1 entries: 1.6 MB
//                  at 200 000 documents, which stay in L2), the row through row_idx, the walk over the term's witness list up to
//                  the first expression that is wanted and true -> keep[m]
//   (k_scan_* of gft_kernels.hip: keep -> rank)
//   k_span_place   a thread an index: span_off[d] = rank[match_off[d]] for d <= n_docs, and the scatter of (start, len, term) of
//                  every kept match whose rank is below the cap
//
//   (text, doc_off, span_off, span_start, span_len, mask)  ->  the text with every span's bytes replaced
//
//   k_redact_check a lane a span: its document by a binary search over span_off, the span against the document's end -> where
//                  its first byte lies (dst[s]); raises ctl[0] for a span that reaches past its document
//   k_redact_fill  returns at once when ctl[0] is raised.  From the output side: a wave a tile of 64 spans, the lengths summed
//                  across the lanes, lane l on virtual byte l + 64 j of the tile; the span of a virtual byte by span_fill_lane
//                  (shuffles only); one byte stored.
//
// Every launch reads only what an earlier launch stored; no atomics.  What a match, a tile and a fill position decide is in
// gft_spans_piece.hpp, which the host compiles too.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gft_kernels.hpp"
#include "gft_spans.hpp"
#include "gft_wave_dev.hpp"

namespace gft {

namespace {

__global__ void __launch_bounds__(kSpanMarkBlock) k_span_mark(const SpanParams P) {
    const uint64_t n_threads = (uint64_t)gridDim.x * kSpanMarkBlock;
    for (uint64_t m = (uint64_t)blockIdx.x * kSpanMarkBlock + threadIdx.x; m < P.n_matches; m += n_threads) {
        const uint64_t d = span_doc_of(P.match_off, P.n_docs, m);
        const uint64_t r = P.row_idx ? P.row_idx[d] : d;
        P.keep[m] = span_match_kept(P.term[m], P.bitmap + r * P.W, P.want, P.wit_off, P.wit_expr);
    }
}

__global__ void __launch_bounds__(kSpanMarkBlock) k_span_place(const SpanParams P) {
    const uint64_t i = (uint64_t)blockIdx.x * kSpanMarkBlock + threadIdx.x;
    if (P.span_off && i <= P.n_docs) P.span_off[i] = P.rank[P.match_off[i]];
    if (i >= P.n_matches || !P.keep[i]) return;
    const uint64_t r = P.rank[i];
    if (r >= P.cap) return;
    const uint32_t t = P.term[i], len = P.term_len[t];
    P.span_start[r] = span_start_of(P.pos[i], len, P.pos_end);
    if (P.span_len) P.span_len[r] = len;
    if (P.span_term) P.span_term[r] = t;
}

__global__ void __launch_bounds__(kSpanMarkBlock) k_redact_check(const RedactParams P) {
    const uint64_t k = (uint64_t)blockIdx.x * kSpanMarkBlock + threadIdx.x;
    if (k >= P.n_spans) return;
    const uint64_t s = P.s0 + k;
    const uint64_t d = span_doc_of(P.span_off, P.n_docs, s);
    const uint64_t a = P.doc_off[d], b = P.doc_off[d + 1];
    const uint32_t start = P.span_start[s];
    if (!redact_span_ok(a, b, start, P.span_len[s])) P.ctl[0] = 1;
    P.dst[k] = a + start;
}

// the prefixes across the lanes as span_fill_lane reads them
struct LaneExcl {
    uint64_t mine;
    __device__ __forceinline__ uint64_t operator()(uint32_t j) const { return shuffle64(mine, (int)j); }
};

__global__ void __launch_bounds__(kSpanMarkBlock) k_redact_fill(const RedactParams P) {
    if (P.ctl[0]) return;                                           // (the same in every lane of the grid: nothing is written)
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t tile = (uint64_t)blockIdx.x * (kSpanMarkBlock / 64) + (threadIdx.x >> 6);
    if (tile >= redact_tiles(P.n_spans)) return;                    // (the same in every lane of a wave)
    const uint64_t k = tile * kSpanTile + lane;
    const uint64_t len = k < P.n_spans ? (uint64_t)P.span_len[P.s0 + k] : 0;
    const uint64_t dst = k < P.n_spans ? P.dst[k] : 0;
    uint64_t incl = len;
#pragma unroll
    for (unsigned by = 1; by < 64; by <<= 1) {
        const uint64_t up = up64(incl, by);
        if (lane >= by) incl += up;
    }
    const LaneExcl excl{incl - len};
    const uint64_t sum = shuffle64(incl, 63);
    const uint8_t mask = (uint8_t)P.mask;
    for (uint64_t base = 0; base < sum; base += 64) {               // (uniform: every lane takes part in the shuffles)
        const uint64_t v = base + lane;
        const uint32_t j = span_fill_lane(excl, v);
        const uint64_t at = shuffle64(dst, (int)j) + (v - excl(j));
        if (v < sum) P.text[at] = mask;
    }
}

}  // namespace

hipError_t launch_span_mark(const SpanParams& P, unsigned n_cus, hipStream_t st) {
    if (!P.n_matches) return hipSuccess;
    const uint64_t blocks = std::min<uint64_t>((P.n_matches + kSpanMarkBlock - 1) / kSpanMarkBlock, (uint64_t)std::max(n_cus, 1u) * 8);
    k_span_mark<<<dim3((unsigned)blocks), dim3(kSpanMarkBlock), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_span_place(const SpanParams& P, hipStream_t st) {
    const uint64_t n = std::max(P.n_docs + 1, P.n_matches);
    k_span_place<<<dim3((unsigned)((n + kSpanMarkBlock - 1) / kSpanMarkBlock)), dim3(kSpanMarkBlock), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_redact_check(const RedactParams& P, hipStream_t st) {
    if (!P.n_spans) return hipSuccess;
    k_redact_check<<<dim3((unsigned)((P.n_spans + kSpanMarkBlock - 1) / kSpanMarkBlock)), dim3(kSpanMarkBlock), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_redact_fill(const RedactParams& P, hipStream_t st) {
    const uint64_t tiles = redact_tiles(P.n_spans);
    if (!tiles) return hipSuccess;
    k_redact_fill<<<dim3((unsigned)((tiles + kSpanMarkBlock / 64 - 1) / (kSpanMarkBlock / 64))), dim3(kSpanMarkBlock), 0, st>>>(P);
    return hipGetLastError();
}

}  // namespace gft
