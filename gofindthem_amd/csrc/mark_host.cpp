// mark_host.cpp -- gft_mark_spans_device's walk on the host (gft_mark.hpp): the runs by the excerpt's host walk with before =
// after = 0 and no snap (excerpt_host.cpp: the same tiles, trips and lanes as the kernels), the check and the place pass of
// gft_mark.hip, and the copy tile by tile, trip by trip and lane by lane through gft_mark_piece.hpp, with the shuffles as array
// reads.  It reads blob[doc_off[0], doc_off[n_docs]) only and asks for no slack.
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/gft.h"
#include "gft_mark.hpp"

namespace gft {

namespace {

struct WindowRel {
    const uint32_t* rel;
    uint32_t operator()(uint32_t w) const { return rel[w]; }
};

// k_mark_copy for one tile
void copy_tile(const MarkPlan& M, const uint8_t* text, const uint64_t* marks, const SelGeom& G, uint64_t tile, uint8_t* out) {
    const uint64_t c0 = tile * (kSelTile / kSelChunk);
    uint64_t tile_lo, tile_hi;
    sel_chunk_range(G, c0, tile_lo, tile_hi);
    const uint64_t nb = mark_count(M, tile_lo);
    uint32_t rel[kMarkWindow];
    for (uint32_t lane = 0; lane < kMarkWindow; lane++) rel[lane] = mark_window_rel(M, nb, lane, tile_lo);
    const uint64_t front = mark_window_front(M, nb);
    for (uint32_t t = 0; t < kSelTrips; t++) {
        for (uint32_t lane = 0; lane < 64; lane++) {
            const uint64_t c = c0 + t * 64u + lane;
            uint64_t lo, hi;
            sel_chunk_range(G, c, lo, hi);
            if (lo >= hi) continue;
            const uint32_t lo_rel = (uint32_t)(lo - tile_lo), hi_rel = (uint32_t)(hi - tile_lo);
            const uint32_t cnt = mark_lift(WindowRel{rel}, lo_rel);
            const bool shown = cnt < kMarkWindow - 1;
            const uint64_t n = shown ? nb + cnt : mark_count(M, lo);
            const uint64_t prev_at = !shown ? mark_at(M, n - 1) : cnt ? tile_lo + rel[cnt - 1] : front;
            const uint32_t j = sel_chunk_byte(G, c, lo);
            const SelV T = mark_chunk_text(M, text, mark_chunk_src(M, n, prev_at, lo), lo, hi);
            SelV acc{0, 0};
            if (shown && mark_chunk_plain(M, n, prev_at, lo, rel[cnt], hi_rel)) acc = sel_shift(T, j);
            else mark_chunk_rest(M, MarkWin{rel, nb, tile_lo}, T, marks, hi, MarkCursor{lo, n, j}, acc);
            sel_store(out, G, c, lo, hi, acc);
        }
    }
}

}  // namespace

int mark_spans_host(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const uint64_t* span_off, const uint32_t* span_start,
                    const uint32_t* span_len, const uint8_t* open, uint32_t open_len, const uint8_t* close, uint32_t close_len, uint32_t flags,
                    uint8_t* out, uint64_t cap_bytes, uint64_t* out_off, uint32_t* span_new, uint64_t* doc_run_off, uint64_t* n_runs,
                    uint64_t* total_bytes) {
    if (n_runs) *n_runs = 0;
    if (total_bytes) *total_bytes = 0;
    if (flags) return GFT_E_INVALID;
    if (open_len > GFT_MARK_MAX || close_len > GFT_MARK_MAX) return GFT_E_INVALID;
    if ((open_len && !open) || (close_len && !close)) return GFT_E_INVALID;
    if (n_docs && (!doc_off || !span_off)) return GFT_E_INVALID;
    if (cap_bytes && !out) return GFT_E_INVALID;
    if (!n_docs) {                                                  // (span_off is not read, as on the device: no span, no text)
        if (out_off) out_off[0] = 0;
        if (doc_run_off) doc_run_off[0] = 0;
        return GFT_OK;
    }
    // the runs: the excerpts of before = after = 0, counted, then with their index arrays; the checks are the excerpt's
    uint64_t m = 0, bytes = 0;
    int rc = excerpt_spans_host(blob, doc_off, n_docs, span_off, span_start, span_len, 0, 0, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0,
                                nullptr, nullptr, &m, &bytes);
    if (rc) return rc;
    const uint64_t s0 = span_off[0], n = span_off[n_docs] - s0, base = doc_off[0];
    if (mark_buffers_overlap(blob, base, doc_off[n_docs], doc_off, n_docs, span_off, span_start, span_len, s0, n, out, cap_bytes, out_off, span_new,
                             doc_run_off))
        return GFT_E_INVALID;
    std::vector<uint64_t> run_off(m + 1), run_doc(m), run_span_off(m + 1), rank(n_docs + 1);
    std::vector<uint32_t> run_start(m);
    rc = excerpt_spans_host(blob, doc_off, n_docs, span_off, span_start, span_len, 0, 0, 0, nullptr, 0, run_off.data(), run_doc.data(),
                            run_start.data(), run_span_off.data(), m, nullptr, rank.data(), &m, &bytes);
    if (rc) return rc;
    // k_mark_check
    for (uint64_t d = 0; d < n_docs; d++)
        if (!mark_grow_ok(doc_off[d + 1] - doc_off[d], rank[d + 1] - rank[d], open_len, close_len)) return GFT_E_INVALID;
    const uint64_t total = (doc_off[n_docs] - base) + m * ((uint64_t)open_len + close_len);
    if (n_runs) *n_runs = m;
    if (total_bytes) *total_bytes = total;
    // k_mark_place
    std::vector<uint64_t> q(2 * m);
    for (uint64_t r = 0; r < m; r++) {
        const uint64_t d = run_doc[r];
        q[2 * r] = doc_off[d] + run_start[r];
        q[2 * r + 1] = q[2 * r] + (run_off[r + 1] - run_off[r]);
        if (span_new)
            for (uint64_t s = run_span_off[r]; s < run_span_off[r + 1]; s++) span_new[s] = mark_span_new(span_start[s], r - rank[d], open_len, close_len);
    }
    for (uint64_t d = 0; d <= n_docs; d++) {
        if (doc_run_off) doc_run_off[d] = rank[d];
        if (out_off) out_off[d] = doc_off[d] - base + rank[d] * ((uint64_t)open_len + close_len);
    }
    // k_mark_copy: bytes [0, min(total, cap_bytes)) of the output
    uint64_t marks[kMarkWords];
    memset(marks, 0, sizeof marks);
    if (open_len) memcpy(marks, open, open_len);
    if (close_len) memcpy(reinterpret_cast<uint8_t*>(marks) + kMarkSlot, close, close_len);
    const MarkPlan M{q.data(), 2 * m, base, doc_off[n_docs] - base, open_len, close_len};
    const SelGeom G = sel_geom(total, cap_bytes, out);
    for (uint64_t tile = 0, tiles = sel_tiles(G); tile < tiles; tile++) copy_tile(M, blob, marks, G, tile, out);
    return GFT_OK;
}

}  // namespace gft
