// select_host.cpp -- gft_select_docs_device's walk on the host (gft_select.hpp): the mark pass, the two prefix sums, the place
// pass and the copy pass of gft_select.hip, tile by tile, trip by trip and lane by lane through gft_select_piece.hpp, with the
// shuffles as array reads and the ballots as loops.  Product code: a finder selects with it when a batch's rows were completed
// on the host.  It reads blob[doc_off[0], doc_off[n_docs]) only and asks for no slack.
#include <algorithm>
#include <vector>

#include "../../include/gft.h"
#include "gft_select.hpp"

namespace gft {

namespace {

// the window across the lanes as sel_lift reads it
struct WindowRel {
    const uint32_t* w;
    uint32_t operator()(uint32_t j) const { return w[j]; }
};

struct Window {
    uint32_t rel[kSelWindow];
    uint64_t delta[kSelWindow];
    void load(const uint64_t* c_off, const uint64_t* c_src, uint64_t m, uint64_t base, uint64_t tile_lo) {
        for (uint32_t lane = 0; lane < kSelWindow; lane++) {
            rel[lane] = sel_window_rel(c_off, m, base, lane, tile_lo);
            delta[lane] = sel_window_delta(c_off, c_src, m, base, lane);
        }
    }
};

// k_select_copy for one tile
void copy_tile(const uint8_t* text, const uint64_t* c_off, const uint64_t* c_src, uint64_t m, const SelGeom& G, uint64_t tile, uint8_t* out) {
    const uint64_t c0 = tile * (kSelTile / kSelChunk);
    uint64_t tile_lo, tile_hi;
    sel_chunk_range(G, c0, tile_lo, tile_hi);
    uint64_t kbase = sel_search(c_off, m, tile_lo);
    Window win;
    win.load(c_off, c_src, m, kbase, tile_lo);
    for (uint32_t t = 0; t < kSelTrips; t++) {
        uint64_t lo[64], hi[64], k[64], doc_delta[64];
        uint32_t doc_end[64];
        bool need[64];
        uint32_t left = 0;
        for (uint32_t lane = 0; lane < 64; lane++) {
            sel_chunk_range(G, c0 + t * 64u + lane, lo[lane], hi[lane]);
            need[lane] = lo[lane] < hi[lane];
            k[lane] = 0; doc_delta[lane] = 0; doc_end[lane] = 0;
            left += need[lane];
        }
        while (left) {
            uint32_t newly = 0, first = 64;
            for (uint32_t lane = 0; lane < 64; lane++) {
                if (!need[lane]) continue;
                const uint32_t idx = sel_lift(WindowRel{win.rel}, (uint32_t)(lo[lane] - tile_lo));
                if (idx < kSelWindow - 1) {
                    k[lane] = kbase + idx; doc_end[lane] = win.rel[idx + 1]; doc_delta[lane] = win.delta[idx];
                    need[lane] = false; newly++; left--;
                } else if (first == 64) {
                    first = lane;
                }
            }
            if (!left) break;
            if (newly) kbase += kSelWindow - 1;
            else kbase = sel_search(c_off, m, lo[first]);
            win.load(c_off, c_src, m, kbase, tile_lo);
        }
        for (uint32_t lane = 0; lane < 64; lane++) {
            if (lo[lane] >= hi[lane]) continue;
            const uint64_t c = c0 + t * 64u + lane;
            SelV acc{0, 0};
            const uint64_t p = sel_segment_at(text, doc_delta[lane], tile_lo + doc_end[lane], lo[lane], hi[lane], sel_chunk_byte(G, c, lo[lane]), acc);
            if (p < hi[lane]) sel_more_segments(text, c_off, c_src, k[lane], p, hi[lane], sel_chunk_byte(G, c, p), acc);
            sel_store(out, G, c, lo[lane], hi[lane], acc);
        }
    }
}

}  // namespace

void select_copy_host(const uint8_t* text, const uint64_t* c_off, const uint64_t* c_src, uint64_t m, const SelGeom& G, uint8_t* out) {
    for (uint64_t tile = 0, n = sel_tiles(G); tile < n; tile++) copy_tile(text, c_off, c_src, m, G, tile, out);
}

bool select_mark_host(const uint64_t* doc_off, uint64_t n_docs, const uint32_t* bitmap, uint32_t W, const uint32_t* wm, uint32_t mode,
                      const uint8_t* also, uint32_t* sel, uint32_t* len) {
    bool good = true;
    for (uint64_t d = 0; d < n_docs; d++) {
        SelRow r{0, 1};
        for (uint32_t j = 0; j < W; j++) r = sel_row_join(r, sel_row_word(bitmap[d * W + j], wm[j]));
        uint32_t s = sel_row_decide(r, mode);
        if (also && also[d]) s = 1;
        const uint32_t ok = sel_doc_ok(doc_off[d], doc_off[d + 1]);
        if (!ok) good = false;
        if (len) len[d] = (s && ok) ? (uint32_t)(doc_off[d + 1] - doc_off[d]) : 0u;
        sel[d] = s;
    }
    return good;
}

int select_docs_host(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const uint32_t* bitmap, uint32_t n_cols,
                     const uint32_t* want, uint32_t mode, const uint8_t* also, uint8_t* out, uint64_t cap_bytes, uint64_t* out_off,
                     uint64_t* doc_idx, uint64_t cap_docs, uint64_t* n_selected, uint64_t* total_bytes) {
    if (n_selected) *n_selected = 0;
    if (total_bytes) *total_bytes = 0;
    const uint32_t W = (n_cols + 31) / 32;
    if (n_docs && (!doc_off || (W && !bitmap))) return GFT_E_INVALID;
    if ((cap_bytes && !out) || (cap_docs && (!out_off || !doc_idx))) return GFT_E_INVALID;
    if (mode != GFT_SELECT_ANY && mode != GFT_SELECT_ALL && mode != GFT_SELECT_NONE) return GFT_E_INVALID;
    if (!n_docs) {
        if (out_off) out_off[0] = 0;
        return GFT_OK;
    }
    std::vector<uint32_t> wm(std::max<uint32_t>(W, 1), 0);
    select_want_words(want, n_cols, wm.data());
    // k_select_mark
    std::vector<uint32_t> len(n_docs), sel(n_docs);
    const bool bad = !select_mark_host(doc_off, n_docs, bitmap, W, wm.data(), mode, also, sel.data(), len.data());
    if (bad) return GFT_E_INVALID;
    if (doc_off[n_docs] > doc_off[0] && !blob) return GFT_E_INVALID;
    if (select_buffers_overlap(blob, doc_off[0], doc_off[n_docs], doc_off, n_docs, bitmap, n_cols, also, out, cap_bytes, out_off, doc_idx,
                               cap_docs))
        return GFT_E_INVALID;
    // the prefix sums
    std::vector<uint64_t> pos(n_docs + 1, 0), rank(n_docs + 1, 0);
    for (uint64_t d = 0; d < n_docs; d++) { pos[d + 1] = pos[d] + len[d]; rank[d + 1] = rank[d] + sel[d]; }
    const uint64_t total = pos[n_docs], m = rank[n_docs];
    if (n_selected) *n_selected = m;
    if (total_bytes) *total_bytes = total;
    // k_select_place
    std::vector<uint64_t> c_off(m + 1), c_src(m);
    const SelPlace O{doc_off, pos.data(), rank.data(), c_off.data(), c_src.data(), out_off, doc_idx, cap_docs};
    sel_place_close(O, m, total);
    for (uint64_t d = 0, r; d < n_docs; d++) sel_place_doc(O, d, r);
    // k_select_copy
    const SelGeom G = sel_geom(total, cap_bytes, out);
    select_copy_host(blob, c_off.data(), c_src.data(), m, G, out);
    return GFT_OK;
}

}  // namespace gft
