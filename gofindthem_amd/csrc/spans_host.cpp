// spans_host.cpp -- the walks of gft_spans.hip on the host (gft_spans.hpp): mark, prefix sum and place over a match CSR, match tile
// by match tile; the redaction's check pass, and its fill pass tile by tile and lane by lane with the shuffles as array reads --
// all through gft_spans_piece.hpp, the search included.  No device, no handle.
#include <algorithm>
#include <vector>

#include "../../include/gft.h"
#include "gft_spans.hpp"

namespace gft {

namespace {
// the prefixes across the lanes as span_fill_lane reads them
struct LaneExcl {
    const uint64_t* v;
    uint64_t operator()(uint32_t j) const { return v[j]; }
};
}  // namespace

int hit_spans_host(const uint64_t* match_off, const uint32_t* term_id, const uint32_t* pos, uint64_t n_docs, const uint32_t* term_len,
                   uint32_t pos_end, const uint64_t* wit_off, const uint32_t* wit_expr, const uint32_t* bitmap, uint32_t n_exprs,
                   const uint64_t* row_idx, const uint32_t* want, uint64_t* span_off, uint32_t* span_start, uint32_t* span_len,
                   uint32_t* span_term, uint64_t cap, uint64_t* total) {
    if (total) *total = 0;
    if (cap && !span_start) return GFT_E_INVALID;
    if (!n_docs) {
        if (span_off) span_off[0] = 0;
        return GFT_OK;
    }
    if (!match_off) return GFT_E_INVALID;
    for (uint64_t d = 0; d < n_docs; d++)
        if (match_off[d] > match_off[d + 1]) return GFT_E_INVALID;
    if (match_off[0] != 0) return GFT_E_INVALID;
    const uint64_t nm = match_off[n_docs];
    const uint32_t W = (n_exprs + 31) / 32;
    if (nm && (!term_id || !pos || !term_len || !wit_off || (W && !bitmap))) return GFT_E_INVALID;
    const ByteRange ins[5] = {{match_off, (n_docs + 1) * 8}, {term_id, nm * 4}, {pos, nm * 4},
                              {bitmap, row_idx ? (uint64_t)W * 4 : n_docs * W * 4}, {row_idx, n_docs * 8}};
    if (spans_outputs_overlap(span_off, n_docs, span_start, span_len, span_term, cap, ins, 5)) return GFT_E_INVALID;
    // k_span_mark, a workgroup's step at a time
    std::vector<uint32_t> keep(nm);
    for (uint64_t m0 = 0; m0 < nm; m0 += kSpanMarkBlock)
        for (uint64_t m = m0; m < std::min<uint64_t>(m0 + kSpanMarkBlock, nm); m++) {
            const uint64_t d = span_doc_of(match_off, n_docs, m);
            const uint64_t r = row_idx ? row_idx[d] : d;
            keep[m] = span_match_kept(term_id[m], bitmap + r * W, want, wit_off, wit_expr);
        }
    // the prefix sum
    std::vector<uint64_t> rank(nm + 1, 0);
    for (uint64_t m = 0; m < nm; m++) rank[m + 1] = rank[m] + keep[m];
    if (total) *total = rank[nm];
    // k_span_place
    for (uint64_t i = 0; i < std::max(n_docs + 1, nm); i++) {
        if (span_off && i <= n_docs) span_off[i] = rank[match_off[i]];
        if (i >= nm || !keep[i]) continue;
        const uint64_t r = rank[i];
        if (r >= cap) continue;
        const uint32_t t = term_id[i], len = term_len[t];
        span_start[r] = span_start_of(pos[i], len, pos_end);
        if (span_len) span_len[r] = len;
        if (span_term) span_term[r] = t;
    }
    return GFT_OK;
}

int redact_spans_host(uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const uint64_t* span_off, const uint32_t* span_start,
                      const uint32_t* span_len, uint32_t mask_byte) {
    if (mask_byte > 255) return GFT_E_INVALID;
    if (!n_docs) return GFT_OK;
    if (!doc_off || !span_off) return GFT_E_INVALID;
    if (span_off[n_docs] < span_off[0]) return GFT_E_INVALID;
    const uint64_t s0 = span_off[0], n = span_off[n_docs] - s0;
    if (!n) return GFT_OK;
    if (!blob || !span_start || !span_len) return GFT_E_INVALID;
    // k_redact_check
    std::vector<uint64_t> dst(n);
    bool bad = false;
    for (uint64_t k = 0; k < n; k++) {
        const uint64_t d = span_doc_of(span_off, n_docs, s0 + k);
        if (!redact_span_ok(doc_off[d], doc_off[d + 1], span_start[s0 + k], span_len[s0 + k])) bad = true;
        dst[k] = doc_off[d] + span_start[s0 + k];
    }
    if (bad) return GFT_E_INVALID;
    // k_redact_fill
    for (uint64_t tile = 0; tile < redact_tiles(n); tile++) {
        uint64_t excl[kSpanTile], at0[kSpanTile], sum = 0;
        for (uint32_t lane = 0; lane < kSpanTile; lane++) {
            const uint64_t k = tile * kSpanTile + lane;
            excl[lane] = sum;
            at0[lane] = k < n ? dst[k] : 0;
            sum += k < n ? span_len[s0 + k] : 0;
        }
        for (uint64_t base = 0; base < sum; base += 64)
            for (uint32_t lane = 0; lane < 64 && base + lane < sum; lane++) {
                const uint64_t v = base + lane;
                const uint32_t j = span_fill_lane(LaneExcl{excl}, v);
                blob[at0[j] + (v - excl[j])] = (uint8_t)mask_byte;
            }
    }
    return GFT_OK;
}

}  // namespace gft
