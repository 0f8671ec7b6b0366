// gft_lowermap.hip -- spans of a lowered batch mapped back to the source text (gft_map_spans_to_source_device), gfx950 / wave64.
//
//   (source text, doc_off, unit table, unit_out, the pieces' table; span_off, span_start, span_len)  ->  the spans, in place
//
//   (k_lower<kLowerTable> of gft_tolower.hip: the pieces' table)
//   k_lowermap_check  a lane a span: its document by a binary search over span_off (span_doc_of, as the redaction's check pass),
//                     the span against the document's lowered length, then lowermap_span: a binary search over the document's
//                     units and one over the unit's pieces for the first and for the last byte, the runes inside the two pieces
//                     from their windows -> mapped[2 k], mapped[2 k + 1]; raises ctl[0] for a span past the lowered end
//   k_lowermap_write  returns at once when ctl[0] is raised; copies mapped into span_start / span_len
//
// Every launch reads only what an earlier launch stored; no atomics.  What a span decides is in gft_lowermap_piece.hpp, which the
// host compiles too.
#include <hip/hip_runtime.h>

#include "gft_lowermap.hpp"

namespace gft {

namespace {

constexpr uint32_t kMapBlock = 256;

__global__ void __launch_bounds__(kMapBlock) k_lowermap_check(const LowerMapParams P) {
    const uint64_t k = (uint64_t)blockIdx.x * kMapBlock + threadIdx.x;
    if (k >= P.n_spans) return;
    const uint64_t s = P.s0 + k;
    const uint64_t d = span_doc_of(P.span_off, P.V.n_docs, s);
    uint32_t a = 0, n = 0;
    if (!lowermap_span(P.V, d, P.span_start[s], P.span_len[s], a, n)) P.ctl[0] = 1;
    P.mapped[2 * k] = a;
    P.mapped[2 * k + 1] = n;
}

__global__ void __launch_bounds__(kMapBlock) k_lowermap_write(const LowerMapParams P) {
    if (P.ctl[0]) return;                                           // (the same in every lane of the grid: nothing is written)
    const uint64_t k = (uint64_t)blockIdx.x * kMapBlock + threadIdx.x;
    if (k >= P.n_spans) return;
    P.span_start[P.s0 + k] = P.mapped[2 * k];
    P.span_len[P.s0 + k] = P.mapped[2 * k + 1];
}

}  // namespace

hipError_t launch_lowermap_check(const LowerMapParams& P, hipStream_t st) {
    if (!P.n_spans) return hipSuccess;
    k_lowermap_check<<<dim3((unsigned)((P.n_spans + kMapBlock - 1) / kMapBlock)), dim3(kMapBlock), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_lowermap_write(const LowerMapParams& P, hipStream_t st) {
    if (!P.n_spans) return hipSuccess;
    k_lowermap_write<<<dim3((unsigned)((P.n_spans + kMapBlock - 1) / kMapBlock)), dim3(kMapBlock), 0, st>>>(P);
    return hipGetLastError();
}

}  // namespace gft
