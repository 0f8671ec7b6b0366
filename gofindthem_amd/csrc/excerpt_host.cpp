// excerpt_host.cpp -- gft_excerpt_spans_device's walk on the host (gft_excerpt.hpp): the document pass, the window pass, the carry
// pass and the mark pass of gft_excerpt.hip tile by tile, trip by trip, wave by wave and lane by lane through
// gft_excerpt_piece.hpp, with the shuffles as array reads; the two prefix sums, the place and the finish pass; the copy excerpt by
// excerpt.  Product code: a finder cuts with it when it does not take the device route.  It reads blob[doc_off[0],
// doc_off[n_docs]) only and asks for no slack.  gft_excerpt_spans_snap_device's walk is the same one with the <true> lane of the
// window pass (excerpt_spans_snap_host); the class table is an argument, so this file links without the table's.
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/gft.h"
#include "gft_excerpt.hpp"

namespace gft {

namespace {

// block_suffix_min of gft_excerpt.hip over the n_waves * 64 values of a workgroup: v -> incl, excl; tot as the kernel leaves it
void block_suffix_min(const uint64_t* v, uint32_t n_waves, uint64_t carry, uint64_t* tot, uint64_t* incl, uint64_t* excl) {
    std::vector<uint64_t> sc(v, v + (size_t)n_waves * 64), nx(sc.size());
    for (uint32_t w = 0; w < n_waves; w++) {
        uint64_t* s = sc.data() + (size_t)w * 64;
        for (uint32_t step = 1; step < 64; step <<= 1) {
            uint64_t t[64];
            for (uint32_t lane = 0; lane < 64; lane++) t[lane] = exc_scan_step(s[lane], s[std::min(lane + step, 63u)], lane, step);
            memcpy(s, t, sizeof t);
        }
        tot[w] = s[0];
    }
    for (uint32_t w = 0; w < n_waves; w++) {
        const uint64_t later = exc_later(tot, n_waves, (int)w, carry);
        for (uint32_t lane = 0; lane < 64; lane++) {
            const uint64_t* s = sc.data() + (size_t)w * 64;
            incl[w * 64 + lane] = exc_min(s[lane], later);
            excl[w * 64 + lane] = exc_exclusive(s[std::min(lane + 1, 63u)], later, lane);
        }
    }
}

// both calls behind their own checks of flags and reach.  V: before, after, flags, reach and the class table are set
int excerpt_walk(ExcView V, const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const uint64_t* span_off, const uint32_t* span_start,
                 const uint32_t* span_len, uint8_t* out, uint64_t cap_bytes, uint64_t* exc_off, uint64_t* exc_doc, uint32_t* exc_start,
                 uint64_t* exc_span_off, uint64_t cap_exc, uint32_t* span_rel, uint64_t* doc_exc_off, uint64_t* n_exc, uint64_t* total_bytes) {
    if (n_docs && (!doc_off || !span_off)) return GFT_E_INVALID;
    if (cap_bytes && !out) return GFT_E_INVALID;
    if (!n_docs) {                                                  // (span_off is not read, as on the device: no span, from index 0)
        if (exc_off) exc_off[0] = 0;
        if (exc_span_off) exc_span_off[0] = 0;
        if (doc_exc_off) doc_exc_off[0] = 0;
        return GFT_OK;
    }
    // k_excerpt_docs
    for (uint64_t d = 0; d < n_docs; d++)
        if (!sel_doc_ok(doc_off[d], doc_off[d + 1]) || span_off[d + 1] < span_off[d]) return GFT_E_INVALID;
    const uint64_t s0 = span_off[0], n = span_off[n_docs] - s0;
    if (n && (!span_start || !span_len)) return GFT_E_INVALID;
    if (doc_off[n_docs] > doc_off[0] && !blob) return GFT_E_INVALID;
    if (excerpt_buffers_overlap(blob, doc_off[0], doc_off[n_docs], doc_off, n_docs, span_off, span_start, span_len, s0, n, out, cap_bytes, exc_off,
                                exc_doc, exc_start, exc_span_off, cap_exc, span_rel, doc_exc_off))
        return GFT_E_INVALID;
    V.text = blob; V.doc_off = doc_off; V.n_docs = n_docs; V.span_off = span_off; V.span_start = span_start; V.span_len = span_len;
    const bool snap = (V.flags & (GFT_EXCERPT_WORDS | GFT_EXCERPT_LINES)) != 0;    // (the instantiation launch_excerpt_window picks)
    const uint64_t n_tiles = exc_tiles(n);
    std::vector<uint64_t> ws(n), we(n), sdoc(n), smin(n), tmin(n_tiles), carry(n_tiles);
    std::vector<uint32_t> head(n), share(n);
    uint64_t lane_v[kExcCarryTiles], incl[kExcCarryTiles], excl[kExcCarryTiles], tot[kExcCarryTiles / 64];
    // k_excerpt_window
    uint64_t bad = 0;
    for (uint64_t tile = 0; tile < n_tiles; tile++) {
        for (uint32_t i = 0; i < kExcTile; i++) {
            const uint64_t k = tile * kExcTile + i;
            lane_v[i] = kExcNone;
            if (k >= n) continue;
            bad |= snap ? exc_lane_window_t<true>(V, s0 + k, sdoc[k], ws[k], we[k]) : exc_lane_window_t<false>(V, s0 + k, sdoc[k], ws[k], we[k]);
            lane_v[i] = ws[k];
        }
        block_suffix_min(lane_v, kExcTile / 64, kExcNone, tot, incl, excl);
        tmin[tile] = incl[0];
    }
    if (bad) return GFT_E_INVALID;
    // k_excerpt_carry
    uint64_t c = kExcNone;
    for (uint64_t trip = exc_trips(n_tiles); trip-- > 0;) {
        for (uint32_t i = 0; i < kExcCarryTiles; i++) {
            const uint64_t t = trip * kExcCarryTiles + i;
            lane_v[i] = t < n_tiles ? tmin[t] : kExcNone;
        }
        block_suffix_min(lane_v, kExcCarryTiles / 64, c, tot, incl, excl);
        for (uint32_t i = 0; i < kExcCarryTiles; i++) {
            const uint64_t t = trip * kExcCarryTiles + i;
            if (t < n_tiles) carry[t] = excl[i];
        }
        c = exc_later(tot, kExcCarryTiles / 64, -1, c);
    }
    // k_excerpt_mark
    for (uint64_t tile = 0; tile < n_tiles; tile++) {
        for (uint32_t i = 0; i < kExcTile; i++) {
            const uint64_t k = tile * kExcTile + i;
            lane_v[i] = k < n ? ws[k] : kExcNone;
        }
        block_suffix_min(lane_v, kExcTile / 64, carry[tile], tot, incl, excl);
        for (uint32_t i = 0; i < kExcTile; i++) {
            const uint64_t k = tile * kExcTile + i;
            if (k >= n) break;
            const bool first = k == 0 || s0 + k == span_off[sdoc[k]];
            const uint64_t prev_we = k ? we[k - 1] : 0;
            smin[k] = incl[i];
            head[k] = exc_is_head(first, prev_we, incl[i]);
            share[k] = exc_share(head[k], we[k], prev_we, incl[i]);
        }
    }
    // the prefix sums
    std::vector<uint64_t> rank(n + 1, 0), pos(n + 1, 0);
    for (uint64_t k = 0; k < n; k++) { rank[k + 1] = rank[k] + head[k]; pos[k + 1] = pos[k] + share[k]; }
    const uint64_t m = rank[n], total = pos[n];
    if (n_exc) *n_exc = m;
    if (total_bytes) *total_bytes = total;
    // k_excerpt_place
    std::vector<uint64_t> c_off(m + 1), c_src(m);
    c_off[m] = total;
    if (exc_off && m <= cap_exc) exc_off[m] = total;
    if (exc_span_off && m <= cap_exc) exc_span_off[m] = s0 + n;
    for (uint64_t k = 0; k < n; k++) {
        if (!head[k]) continue;
        const uint64_t r = rank[k], d = sdoc[k];
        c_off[r] = pos[k];
        c_src[r] = smin[k];
        if (r <= cap_exc) {
            if (exc_off) exc_off[r] = pos[k];
            if (exc_span_off) exc_span_off[r] = s0 + k;
        }
        if (r < cap_exc) {
            if (exc_doc) exc_doc[r] = d;
            if (exc_start) exc_start[r] = (uint32_t)(smin[k] - doc_off[d]);
        }
    }
    // k_excerpt_finish
    if (span_rel)
        for (uint64_t k = 0; k < n; k++)
            span_rel[s0 + k] = (uint32_t)(doc_off[sdoc[k]] + span_start[s0 + k] - c_src[rank[k] + head[k] - 1]);
    if (doc_exc_off)
        for (uint64_t d = 0; d <= n_docs; d++) doc_exc_off[d] = rank[span_off[d] - s0];
    // the copy: bytes [0, min(total, cap_bytes)) of the output
    const uint64_t end = std::min(total, cap_bytes);
    for (uint64_t r = 0; r < m && c_off[r] < end; r++) {
        const uint64_t len = std::min(c_off[r + 1], end) - c_off[r];
        if (len) memcpy(out + c_off[r], blob + c_src[r], (size_t)len);
    }
    return GFT_OK;
}

}  // namespace

int excerpt_spans_host(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const uint64_t* span_off, const uint32_t* span_start,
                       const uint32_t* span_len, uint32_t before, uint32_t after, uint32_t flags, uint8_t* out, uint64_t cap_bytes,
                       uint64_t* exc_off, uint64_t* exc_doc, uint32_t* exc_start, uint64_t* exc_span_off, uint64_t cap_exc, uint32_t* span_rel,
                       uint64_t* doc_exc_off, uint64_t* n_exc, uint64_t* total_bytes) {
    if (n_exc) *n_exc = 0;
    if (total_bytes) *total_bytes = 0;
    if (flags & ~(uint32_t)GFT_EXCERPT_RUNES) return GFT_E_INVALID;
    ExcView V{};
    V.before = before; V.after = after; V.flags = flags;
    return excerpt_walk(V, blob, doc_off, n_docs, span_off, span_start, span_len, out, cap_bytes, exc_off, exc_doc, exc_start, exc_span_off, cap_exc,
                        span_rel, doc_exc_off, n_exc, total_bytes);
}

int excerpt_spans_snap_host(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const uint64_t* span_off, const uint32_t* span_start,
                            const uint32_t* span_len, uint32_t before, uint32_t after, uint32_t flags, uint32_t reach, const WordTable& words,
                            uint8_t* out, uint64_t cap_bytes, uint64_t* exc_off, uint64_t* exc_doc, uint32_t* exc_start, uint64_t* exc_span_off,
                            uint64_t cap_exc, uint32_t* span_rel, uint64_t* doc_exc_off, uint64_t* n_exc, uint64_t* total_bytes) {
    if (n_exc) *n_exc = 0;
    if (total_bytes) *total_bytes = 0;
    if (!exc_snap_args_ok(flags, reach)) return GFT_E_INVALID;
    ExcView V{};
    V.before = before; V.after = after; V.flags = flags; V.reach = reach; V.words = words;
    return excerpt_walk(V, blob, doc_off, n_docs, span_off, span_start, span_len, out, cap_bytes, exc_off, exc_doc, exc_start, exc_span_off, cap_exc,
                        span_rel, doc_exc_off, n_exc, total_bytes);
}

}  // namespace gft
