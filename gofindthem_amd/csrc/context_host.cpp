// context_host.cpp -- gft_context_docs_device's walk on the host (gft_context.hpp): the mark pass, the reach, carry and decide
// passes of gft_context.hip tile by tile, block by block and lane by lane through gft_context_piece.hpp -- the ballots and the
// wave's running extrema as loops --, the three prefix sums, the place pass and the select's copy walk.  Product code: a finder
// takes it when a batch's rows were completed on the host.  It reads blob[doc_off[0], doc_off[n_docs]) only and asks for no slack.
#include <algorithm>
#include <vector>

#include "../../include/gft.h"
#include "gft_context.hpp"

namespace gft {

int context_docs_host(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const uint32_t* bitmap, uint32_t n_cols,
                      const uint32_t* want, uint32_t mode, const uint8_t* also, uint64_t before, uint64_t after, const uint8_t* fence,
                      uint8_t* out, uint64_t cap_bytes, uint64_t* out_off, uint64_t* doc_idx, uint8_t* kind, uint64_t cap_docs,
                      uint64_t* group_off, uint64_t cap_groups, uint64_t* n_kept, uint64_t* n_hits, uint64_t* n_groups, uint64_t* total_bytes) {
    if (n_kept) *n_kept = 0;
    if (n_hits) *n_hits = 0;
    if (n_groups) *n_groups = 0;
    if (total_bytes) *total_bytes = 0;
    const uint32_t W = (n_cols + 31) / 32;
    if (n_docs && (!doc_off || (W && !bitmap))) return GFT_E_INVALID;
    if ((cap_bytes && !out) || (cap_docs && (!out_off || !doc_idx || !kind)) || (cap_groups && !group_off)) return GFT_E_INVALID;
    if (mode != GFT_SELECT_ANY && mode != GFT_SELECT_ALL && mode != GFT_SELECT_NONE) return GFT_E_INVALID;
    if (!n_docs) {
        if (out_off) out_off[0] = 0;
        if (group_off) group_off[0] = 0;
        return GFT_OK;
    }
    std::vector<uint32_t> wm(std::max<uint32_t>(W, 1), 0);
    select_want_words(want, n_cols, wm.data());
    // k_select_mark
    std::vector<uint32_t> sel(n_docs);
    const bool bad = !select_mark_host(doc_off, n_docs, bitmap, W, wm.data(), mode, also, sel.data(), nullptr);
    if (bad) return GFT_E_INVALID;
    if (doc_off[n_docs] > doc_off[0] && !blob) return GFT_E_INVALID;
    if (context_buffers_overlap(blob, doc_off[0], doc_off[n_docs], doc_off, n_docs, bitmap, n_cols, also, fence, out, cap_bytes, out_off, doc_idx,
                                kind, cap_docs, group_off, cap_groups))
        return GFT_E_INVALID;
    // k_ctx_reach
    const uint64_t n_tiles = ctx_tiles(n_docs), n_blocks = ctx_blocks(n_tiles);
    std::vector<uint64_t> word_sel(n_tiles), word_fence(n_tiles), sum(4 * n_tiles), carry(4 * n_tiles), part(5 * n_blocks);
    for (uint64_t t = 0; t < n_tiles; t++) {
        const uint64_t base = t * kCtxTile;
        uint64_t S = 0, F = 0;
        for (uint32_t lane = 0; lane < kCtxTile && base + lane < n_docs; lane++) {
            if (sel[base + lane]) S |= 1ull << lane;
            if (fence && fence[base + lane]) F |= 1ull << lane;
        }
        word_sel[t] = S; word_fence[t] = F;
        sum[t] = ctx_last(S, base); sum[n_tiles + t] = ctx_last(F, base);
        sum[2 * n_tiles + t] = ctx_first(S, base); sum[3 * n_tiles + t] = ctx_first(F, base);
    }
    // k_ctx_carry_blocks
    for (uint64_t b = 0; b < n_blocks; b++) {
        uint64_t all[4] = {0, 0, kCtxNone, kCtxNone}, cnt = 0;
        for (uint64_t t = b * kCtxCarry; t < std::min<uint64_t>((b + 1) * kCtxCarry, n_tiles); t++) {
            all[0] = ctx_max(all[0], sum[t]); all[1] = ctx_max(all[1], sum[n_tiles + t]);
            all[2] = ctx_min(all[2], sum[2 * n_tiles + t]); all[3] = ctx_min(all[3], sum[3 * n_tiles + t]);
            cnt += (uint64_t)__builtin_popcountll(word_sel[t]);
        }
        for (uint32_t k = 0; k < 4; k++) part[k * n_blocks + b] = all[k];
        part[4 * n_blocks + b] = cnt;
    }
    // k_ctx_carry_spine: exclusive, in place
    uint64_t hits = 0;
    {
        uint64_t cs = 0, cf = 0;
        for (uint64_t b = 0; b < n_blocks; b++) {
            const uint64_t s = part[b], f = part[n_blocks + b];
            part[b] = cs; part[n_blocks + b] = cf;
            cs = ctx_max(cs, s); cf = ctx_max(cf, f);
            hits += part[4 * n_blocks + b];
        }
        cs = kCtxNone; cf = kCtxNone;
        for (uint64_t b = n_blocks; b-- > 0;) {
            const uint64_t s = part[2 * n_blocks + b], f = part[3 * n_blocks + b];
            part[2 * n_blocks + b] = cs; part[3 * n_blocks + b] = cf;
            cs = ctx_min(cs, s); cf = ctx_min(cf, f);
        }
    }
    // k_ctx_carry_tiles
    for (uint64_t b = 0; b < n_blocks; b++) {
        const uint64_t t0 = b * kCtxCarry, t1 = std::min<uint64_t>((b + 1) * kCtxCarry, n_tiles);
        uint64_t cs = part[b], cf = part[n_blocks + b];
        for (uint64_t t = t0; t < t1; t++) {
            carry[t] = cs; carry[n_tiles + t] = cf;
            cs = ctx_max(cs, sum[t]); cf = ctx_max(cf, sum[n_tiles + t]);
        }
        cs = part[2 * n_blocks + b]; cf = part[3 * n_blocks + b];
        for (uint64_t t = t1; t-- > t0;) {
            carry[2 * n_tiles + t] = cs; carry[3 * n_tiles + t] = cf;
            cs = ctx_min(cs, sum[2 * n_tiles + t]); cf = ctx_min(cf, sum[3 * n_tiles + t]);
        }
    }
    // k_ctx_decide
    std::vector<uint32_t> keep(n_docs), len(n_docs), newgroup(n_docs);
    for (uint64_t t = 0; t < n_tiles; t++) {
        const uint64_t base = t * kCtxTile, S = word_sel[t], F = word_fence[t];
        const CtxCarry c{carry[t], carry[n_tiles + t], carry[2 * n_tiles + t], carry[3 * n_tiles + t]};
        uint64_t K = 0;
        for (uint32_t lane = 0; lane < kCtxTile && base + lane < n_docs; lane++)
            if (ctx_keep(S, F, c, base, lane, before, after)) K |= 1ull << lane;
        for (uint32_t lane = 0; lane < kCtxTile && base + lane < n_docs; lane++) {
            const uint64_t d = base + lane;
            const uint32_t k = (uint32_t)(K >> lane) & 1u;
            const uint32_t left = lane ? (uint32_t)(K >> (lane - 1)) & 1u : (base ? ctx_keep_left(S, F, c, base, before, after) : 0u);
            keep[d] = k;
            len[d] = k ? (uint32_t)(doc_off[d + 1] - doc_off[d]) : 0u;
            newgroup[d] = ctx_new_group(k, left, d, (uint32_t)(F >> lane) & 1u);
        }
    }
    // the prefix sums
    std::vector<uint64_t> pos(n_docs + 1, 0), rank(n_docs + 1, 0), grank(n_docs + 1, 0);
    for (uint64_t d = 0; d < n_docs; d++) {
        pos[d + 1] = pos[d] + len[d]; rank[d + 1] = rank[d] + keep[d]; grank[d + 1] = grank[d] + newgroup[d];
    }
    const uint64_t total = pos[n_docs], m = rank[n_docs], groups = grank[n_docs];
    if (n_kept) *n_kept = m;
    if (n_hits) *n_hits = hits;
    if (n_groups) *n_groups = groups;
    if (total_bytes) *total_bytes = total;
    // k_ctx_place
    std::vector<uint64_t> c_off(m + 1), c_src(m);
    const SelPlace O{doc_off, pos.data(), rank.data(), c_off.data(), c_src.data(), out_off, doc_idx, cap_docs};
    sel_place_close(O, m, total);
    if (group_off && groups <= cap_groups) group_off[groups] = m;
    for (uint64_t d = 0, r; d < n_docs; d++) {
        if (!sel_place_doc(O, d, r)) continue;
        if (r < cap_docs) kind[r] = (uint8_t)((word_sel[d / kCtxTile] >> (d % kCtxTile)) & 1u);
        const uint64_t g = grank[d];
        if (grank[d + 1] != g && group_off && g <= cap_groups) group_off[g] = r;
    }
    // k_select_copy
    const SelGeom G = sel_geom(total, cap_bytes, out);
    select_copy_host(blob, c_off.data(), c_src.data(), m, G, out);
    return GFT_OK;
}

}  // namespace gft
