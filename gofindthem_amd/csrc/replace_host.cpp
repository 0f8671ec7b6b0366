// replace_host.cpp -- gft_replace_spans_device's walk on the host (gft_replace.hpp): the runs by the excerpt's host walk with
// before = after = 0 and no snap (excerpt_host.cpp: the same tiles, trips and lanes as the kernels), the ids, the check and the
// place pass of gft_replace.hip, and the copy tile by tile, trip by trip and lane by lane through gft_replace_piece.hpp, with the
// shuffles and the LDS window as array reads.  It reads blob[doc_off[0], doc_off[n_docs]) only and asks for no slack.
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/gft.h"
#include "gft_replace.hpp"

namespace gft {

namespace {

struct WindowRel {
    const uint32_t* rel;
    uint32_t operator()(uint32_t w) const { return rel[w]; }
};

// k_replace_copy for one tile
void copy_tile(const RepPlan& R, const uint8_t* text, const uint8_t* tab, const SelGeom& G, uint64_t tile, uint8_t* out) {
    const uint64_t c0 = tile * (kSelTile / kSelChunk);
    uint64_t tile_lo, tile_hi, l;
    sel_chunk_range(G, c0, tile_lo, tile_hi);
    sel_chunk_range(G, c0 + kSelTile / kSelChunk - 1, l, tile_hi);
    const uint64_t nb = rep_count(R, tile_lo);
    const uint32_t span = (uint32_t)(tile_hi - tile_lo);
    uint32_t rel[kRepWindow], wlen[kRepWindow], wroff[kRepWindow];
    uint64_t wdelta[kRepWindow];
    for (uint32_t lane = 0; lane < kRepWindow; lane++) {
        rel[lane] = rep_window_rel(R, nb, lane, tile_lo);
        wdelta[lane] = 0; wlen[lane] = wroff[lane] = 0;
        if (rel[lane] < span) { wdelta[lane] = R.delta[nb + lane]; wlen[lane] = R.len[nb + lane]; wroff[lane] = R.roff[nb + lane]; }
    }
    const RepEntry front = nb ? rep_entry(R, nb - 1) : rep_entry_none(R);
    const RepWin W{rel, wdelta, wlen, wroff, nb, tile_lo, span, front};
    const bool easy = front.at + front.len <= tile_lo && rel[0] >= span;
    uint64_t lo[kSelTrips][64], hi[kSelTrips][64];
    RepCursor cur[kSelTrips][64];
    SelV acc[kSelTrips][64];
    for (uint32_t t = 0; t < kSelTrips; t++) {
        for (uint32_t lane = 0; lane < 64; lane++) {
            const uint64_t c = c0 + t * 64u + lane;
            uint64_t& a = lo[t][lane];
            uint64_t& b = hi[t][lane];
            sel_chunk_range(G, c, a, b);
            acc[t][lane] = SelV{0, 0};
            cur[t][lane] = RepCursor{b, 0, 0};
            if (a >= b) continue;
            const uint32_t j = sel_chunk_byte(G, c, a);
            if (easy) { acc[t][lane] = sel_shift(sel_load(text + (front.delta + a), (uint32_t)(b - a)), j); continue; }
            const uint32_t lo_rel = (uint32_t)(a - tile_lo), hi_rel = (uint32_t)(b - tile_lo);
            const uint32_t cnt = mark_lift(WindowRel{rel}, lo_rel);
            if (cnt < kRepWindow - 1) {
                const RepEntry E = cnt ? RepEntry{tile_lo + rel[cnt - 1], wdelta[cnt - 1], wlen[cnt - 1], wroff[cnt - 1]} : front;
                if (rep_chunk_plain(E, a, rel[cnt], hi_rel)) acc[t][lane] = sel_shift(sel_load(text + (E.delta + a), (uint32_t)(b - a)), j);
                else cur[t][lane] = RepCursor{a, nb + cnt, j};
            } else {
                cur[t][lane] = RepCursor{a, rep_count(R, a), j};
            }
        }
    }
    // step k: the k-th segment of every chunk of the tile
    for (bool more = true; more;) {
        more = false;
        for (uint32_t t = 0; t < kSelTrips; t++)
            for (uint32_t lane = 0; lane < 64; lane++)
                if (cur[t][lane].p < hi[t][lane]) {
                    rep_segment(R, W, text, tab, hi[t][lane], cur[t][lane], acc[t][lane]);
                    more |= cur[t][lane].p < hi[t][lane];
                }
    }
    for (uint32_t t = 0; t < kSelTrips; t++)
        for (uint32_t lane = 0; lane < 64; lane++)
            if (lo[t][lane] < hi[t][lane]) sel_store(out, G, c0 + t * 64u + lane, lo[t][lane], hi[t][lane], acc[t][lane]);
}

}  // namespace

int replace_spans_host(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const uint64_t* span_off, const uint32_t* span_start,
                       const uint32_t* span_len, const uint32_t* span_key, const uint32_t* key_rep, uint32_t n_keys, const uint8_t* rep_bytes,
                       const uint64_t* rep_off, uint32_t n_reps, uint32_t flags, uint8_t* out, uint64_t cap_bytes, uint64_t* out_off,
                       uint64_t* doc_run_off, uint32_t* run_new, uint32_t* run_len, uint32_t* run_rep, uint64_t cap_runs, uint64_t* n_runs,
                       uint64_t* total_bytes) {
    if (n_runs) *n_runs = 0;
    if (total_bytes) *total_bytes = 0;
    if (flags) return GFT_E_INVALID;
    if (!replace_table_ok(rep_bytes, rep_off, n_reps)) return GFT_E_INVALID;
    if (n_docs && (!doc_off || !span_off)) return GFT_E_INVALID;
    if (cap_bytes && !out) return GFT_E_INVALID;
    if (cap_runs > (~0ull >> 4)) return GFT_E_INVALID;
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
    if (replace_buffers_overlap(blob, base, doc_off[n_docs], doc_off, n_docs, span_off, span_start, span_len, span_key, s0, n, out, cap_bytes, out_off,
                                doc_run_off, run_new, run_len, run_rep, cap_runs))
        return GFT_E_INVALID;
    std::vector<uint64_t> run_off(m + 1), run_doc(m), run_span_off(m + 1), rank(n_docs + 1);
    std::vector<uint32_t> run_start(m);
    rc = excerpt_spans_host(blob, doc_off, n_docs, span_off, span_start, span_len, 0, 0, 0, nullptr, 0, run_off.data(), run_doc.data(),
                            run_start.data(), run_span_off.data(), m, nullptr, rank.data(), &m, &bytes);
    if (rc) return rc;
    // k_replace_ids: every span's id, the minimum per run
    std::vector<uint32_t> rid(m, kRepNoId);
    for (uint64_t r = 0; r < m; r++)
        for (uint64_t s = run_span_off[r]; s < run_span_off[r + 1]; s++) {
            const uint32_t id = rep_span_id(span_key, key_rep, n_keys, n_reps, s);
            if (id == kRepNoId) return GFT_E_INVALID;
            rid[r] = std::min(rid[r], id);
        }
    // k_replace_len, the prefix sums, k_replace_check
    std::vector<uint64_t> cut(m + 1, 0), put(m + 1, 0);
    for (uint64_t r = 0; r < m; r++) {
        cut[r + 1] = cut[r] + (run_off[r + 1] - run_off[r]);
        put[r + 1] = put[r] + (rep_off[rid[r] + 1] - rep_off[rid[r]]);
    }
    for (uint64_t d = 0; d < n_docs; d++)
        if (!rep_grow_ok(doc_off[d + 1] - doc_off[d], cut[rank[d + 1]] - cut[rank[d]], put[rank[d + 1]] - put[rank[d]])) return GFT_E_INVALID;
    const uint64_t total = (doc_off[n_docs] - base) - cut[m] + put[m];
    if (n_runs) *n_runs = m;
    if (total_bytes) *total_bytes = total;
    // k_replace_place
    std::vector<uint64_t> at(m), delta(m);
    std::vector<uint32_t> len(m), roff(m);
    for (uint64_t r = 0; r < m; r++) {
        const uint64_t d = run_doc[r], q0 = doc_off[d] + run_start[r];
        at[r] = q0 - base + put[r] - cut[r];
        len[r] = (uint32_t)(put[r + 1] - put[r]);
        roff[r] = (uint32_t)rep_off[rid[r]];
        delta[r] = base + cut[r + 1] - put[r + 1];
        if (r < cap_runs) {
            if (run_new) run_new[r] = (uint32_t)(at[r] - (doc_off[d] - base + put[rank[d]] - cut[rank[d]]));
            if (run_len) run_len[r] = len[r];
            if (run_rep) run_rep[r] = rid[r];
        }
    }
    for (uint64_t d = 0; d <= n_docs; d++) {
        if (doc_run_off) doc_run_off[d] = rank[d];
        if (out_off) out_off[d] = doc_off[d] - base + put[rank[d]] - cut[rank[d]];
    }
    // k_replace_copy: bytes [0, min(total, cap_bytes)) of the output
    std::vector<uint8_t> tab((size_t)rep_off[n_reps] + kRepTableSlack, 0);
    if (rep_off[n_reps]) memcpy(tab.data(), rep_bytes, rep_off[n_reps]);
    const RepPlan R{at.data(), delta.data(), len.data(), roff.data(), m, base};
    const SelGeom G = sel_geom(total, cap_bytes, out);
    for (uint64_t tile = 0, tiles = sel_tiles(G); tile < tiles; tile++) copy_tile(R, blob, tab.data(), G, tile, out);
    return GFT_OK;
}

}  // namespace gft
