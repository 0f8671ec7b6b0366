// route_host.cpp -- gft_route_docs_device's walk on the host (gft_route.hpp): the mark pass, the count pass, the prefix sum of the
// (bucket, tile) counts, the place pass and the prefix sum of the entry lengths of gft_route.hip, tile by tile and lane by lane
// through gft_route_piece.hpp with the ballots as loops, then the select's copy walk over the compact arrays.  Product code: a
// finder routes with it when it does not take the device route.  It reads blob[doc_off[0], doc_off[n_docs]) only.
#include <algorithm>
#include <vector>

#include "../../include/gft.h"
#include "gft_route.hpp"

namespace gft {

namespace {

// the ballot of bit b over a tile's lanes
uint64_t tile_ballot(const std::vector<uint64_t>& member, uint64_t n_docs, uint64_t tile, uint32_t b) {
    uint64_t ballot = 0;
    for (uint32_t lane = 0; lane < kRouteTileDocs; lane++) {
        const uint64_t d = tile * kRouteTileDocs + lane;
        if (d < n_docs && ((member[d] >> b) & 1ull)) ballot |= 1ull << lane;
    }
    return ballot;
}

}  // namespace

int route_docs_host(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const uint32_t* bitmap, uint32_t n_cols,
                    const uint32_t* masks, uint32_t n_buckets, uint32_t mode, uint32_t flags, const uint8_t* also, uint8_t* out,
                    uint64_t cap_bytes, uint64_t* out_off, uint64_t* doc_idx, uint64_t cap_docs, uint64_t* bucket_doc, uint64_t* bucket_byte) {
    if (flags & ~GFT_ROUTE_REST) return GFT_E_INVALID;
    const uint32_t rest = (flags & GFT_ROUTE_REST) ? 1u : 0u;
    if (n_buckets > GFT_ROUTE_MAX_BUCKETS - rest) return GFT_E_UNSUPPORTED;
    const uint32_t B = n_buckets + rest, W = (n_cols + 31) / 32;
    for (uint32_t b = 0; b <= B; b++) {
        if (bucket_doc) bucket_doc[b] = 0;
        if (bucket_byte) bucket_byte[b] = 0;
    }
    if (n_docs && (!doc_off || (W && !bitmap))) return GFT_E_INVALID;
    if (n_buckets && W && !masks) return GFT_E_INVALID;
    if ((cap_bytes && !out) || (cap_docs && (!out_off || !doc_idx))) return GFT_E_INVALID;
    if (mode != GFT_ROUTE_FIRST && mode != GFT_ROUTE_EVERY) return GFT_E_INVALID;
    if (also && !rest) return GFT_E_INVALID;
    if (!n_docs) {
        if (out_off) out_off[0] = 0;
        return GFT_OK;
    }
    std::vector<uint32_t> mw(std::max<uint64_t>((uint64_t)n_buckets * W, 1), 0);
    if (W) route_mask_words(masks, n_buckets, n_cols, mw.data());
    // k_route_mark
    std::vector<uint64_t> member(n_docs);
    std::vector<uint32_t> len(n_docs);
    bool bad = false;
    for (uint64_t d = 0; d < n_docs; d++) {
        uint64_t hits = 0;
        for (uint32_t j = 0; j < W; j++) {
            const uint32_t w = bitmap[d * W + j];
            if (w)
                for (uint32_t k = 0; k < n_buckets; k++) hits |= route_word_bit(w, mw[(uint64_t)k * W + j], k);
        }
        const uint32_t ok = sel_doc_ok(doc_off[d], doc_off[d + 1]);
        if (!ok) bad = true;
        len[d] = ok ? (uint32_t)(doc_off[d + 1] - doc_off[d]) : 0u;
        member[d] = route_member(hits, n_buckets, mode, rest, (also && also[d]) ? 1u : 0u);
    }
    if (bad) return GFT_E_INVALID;
    if (doc_off[n_docs] > doc_off[0] && !blob) return GFT_E_INVALID;
    if (route_buffers_overlap(blob, doc_off[0], doc_off[n_docs], doc_off, n_docs, bitmap, n_cols, masks, n_buckets, also, out, cap_bytes, out_off,
                              doc_idx, cap_docs, bucket_doc, bucket_byte, B))
        return GFT_E_INVALID;
    // k_route_count: a tile of 64 documents, a bucket a ballot
    const uint64_t n_tiles = route_tiles(n_docs);
    std::vector<uint32_t> cnt((uint64_t)B * n_tiles);
    uint64_t total = 0;
    for (uint64_t tile = 0; tile < n_tiles; tile++) {
        for (uint32_t b = 0; b < B; b++) cnt[route_cell(b, n_tiles, tile)] = route_popcount(tile_ballot(member, n_docs, tile, b));
        for (uint32_t lane = 0; lane < kRouteTileDocs; lane++) {
            const uint64_t d = tile * kRouteTileDocs + lane;
            if (d < n_docs) total += route_doc_bytes(len[d], member[d]);
        }
    }
    // the prefix sum of the counts: every (bucket, tile) base, the borders, m
    std::vector<uint64_t> base(cnt.size() + 1, 0);
    for (uint64_t i = 0; i < cnt.size(); i++) base[i + 1] = base[i] + cnt[i];
    const uint64_t m = base[cnt.size()];
    // k_route_place
    std::vector<uint32_t> ent_len(m);
    std::vector<uint64_t> c_src(m), c_off(m + 1, 0);
    for (uint64_t tile = 0; tile < n_tiles; tile++) {
        for (uint32_t b = 0; b < B; b++) {
            const uint64_t ballot = tile_ballot(member, n_docs, tile, b);
            if (!ballot) continue;
            for (uint32_t lane = 0; lane < kRouteTileDocs; lane++) {
                if (!((ballot >> lane) & 1ull)) continue;
                const uint64_t d = tile * kRouteTileDocs + lane;
                const uint64_t r = route_rank(base[route_cell(b, n_tiles, tile)], ballot, lane);
                ent_len[r] = len[d];
                c_src[r] = doc_off[d];
                if (r < cap_docs) doc_idx[r] = d;
            }
        }
    }
    // the prefix sum of the entry lengths; k_route_finish
    for (uint64_t r = 0; r < m; r++) c_off[r + 1] = c_off[r] + ent_len[r];
    if (out_off)
        for (uint64_t r = 0; r <= m && r <= cap_docs; r++) out_off[r] = c_off[r];
    for (uint32_t b = 0; b <= B; b++) {
        const uint64_t at = base[route_cell(b, n_tiles, 0)];
        if (bucket_doc) bucket_doc[b] = at;
        if (bucket_byte) bucket_byte[b] = c_off[at];
    }
    // k_select_copy
    const SelGeom G = sel_geom(total, cap_bytes, out);
    select_copy_host(blob, c_off.data(), c_src.data(), m, G, out);
    return GFT_OK;
}

}  // namespace gft
