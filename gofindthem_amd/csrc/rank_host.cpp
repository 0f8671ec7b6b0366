// rank_host.cpp -- the walks of gft_score_docs_device, gft_top_docs_device and gft_gather_docs_device on the host (gft_rank.hpp): the
// score pass workgroup by workgroup, step by step and lane by lane through gft_rank_piece.hpp, with the step's set, the large path's
// bitset and the step's sums as arrays; the select pass by pass with the pick's wave lane by lane; the place pass tile by tile, row
// by row; the sort's network stage by stage; the gather's place pass, prefix sum and the select's copy pass.  No HIP.
#include <algorithm>
#include <vector>

#include "../../include/gft.h"
#include "gft_rank.hpp"
#include "gft_select.hpp"

namespace gft {

namespace {

constexpr uint64_t kHostResident = 512;     // workgroups the host walk cuts a list into at most

inline uint32_t weight_of(const uint32_t* weights, uint32_t t) { return weights ? weights[t] : 1u; }

// k_score_docs for workgroup w of G
void score_group(const uint64_t* off, const uint32_t* term, uint64_t n_docs, uint32_t n_terms, const uint32_t* weights, bool distinct, uint64_t w,
                 uint64_t G, uint64_t* score, uint64_t& top, std::vector<uint64_t>& set, std::vector<uint32_t>& bits) {
    const uint64_t dlo = stats_cut(off, n_docs, w, G), dhi = stats_cut(off, n_docs, w + 1, G);
    std::vector<uint32_t> rel(kStatsStepDocs + 1);
    std::vector<uint64_t> sum(kStatsStepDocs);
    for (uint64_t d = dlo; d < dhi;) {
        const uint64_t e0 = off[d];
        const uint32_t tries = (uint32_t)std::min<uint64_t>(kStatsStepDocs, dhi - d);
        for (uint32_t k = 0; k <= tries; k++) rel[k] = stats_rel(off[d + k], e0);
        for (uint32_t k = 0; k < tries; k++) sum[k] = 0;
        const uint32_t nd = stats_step_docs(rel, tries);
        if (nd) {
            const uint32_t ne = rel[nd];
            std::vector<uint32_t> mine;
            // the lanes in the order the device's trips take the entries: trip major, lane minor
            for (uint32_t i = 0; i < ne; i++) {
                const uint32_t t = term[e0 + i], dl = stats_find_doc(rel, nd, i);
                if (distinct) {
                    const uint64_t key = stats_set_key(dl, t);
                    bool fst = false;
                    for (uint32_t s = stats_set_slot(dl, t);; s = stats_set_next(s)) {
                        if (set[s] == 0) { set[s] = key; fst = true; mine.push_back(s); break; }
                        if (set[s] == key) break;
                    }
                    if (!fst) continue;
                }
                sum[dl] += weight_of(weights, t);
            }
            for (uint32_t s : mine) set[s] = 0;
            for (uint32_t k = 0; k < nd; k++) { score[d + k] = sum[k]; top = std::max(top, sum[k]); }
            d += nd;
        } else {
            const uint64_t cnt = off[d + 1] - e0;
            uint32_t* const b = stats_bitset_in_lds(n_terms) ? reinterpret_cast<uint32_t*>(set.data()) : bits.data();
            uint64_t lane_acc[kRankBlock] = {0};
            for (uint64_t i = 0; i < cnt; i++) {
                const uint32_t t = term[e0 + i], bit = 1u << (t & 31u);
                if (distinct) {
                    const bool fst = !(b[t >> 5] & bit);
                    b[t >> 5] |= bit;
                    if (!fst) continue;
                }
                lane_acc[i % kRankBlock] += weight_of(weights, t);
            }
            if (distinct)
                for (uint64_t i = 0; i < cnt; i++) b[term[e0 + i] >> 5] = 0;
            uint64_t v = 0;
            for (uint32_t l = 0; l < kRankBlock; l++) v += lane_acc[l];
            score[d] = v;
            top = std::max(top, v);
            d += 1;
        }
    }
}

}  // namespace

int score_docs_host(const uint64_t* off, const uint32_t* term, uint64_t n_docs, uint32_t n_terms, const uint32_t* weights, uint32_t flags,
                    uint64_t* score, uint64_t* max_score) {
    if (flags & ~GFT_SCORE_DISTINCT) return GFT_E_INVALID;
    if (n_docs && (!off || !score)) return GFT_E_INVALID;
    if (n_docs > (~0ull >> 4)) return GFT_E_INVALID;
    const uint64_t e0 = n_docs ? off[0] : 0, e1 = n_docs ? off[n_docs] : 0;
    if (e1 < e0 || e1 - e0 > (~0ull >> 4)) return GFT_E_INVALID;
    const uint64_t n = e1 - e0;
    if (n && (!term || !n_terms)) return GFT_E_INVALID;
    if (score_buffers_overlap(off, n_docs, term, e0, n, score)) return GFT_E_INVALID;
    // k_stats_check
    for (uint64_t d = 0; d < n_docs; d++)
        if (off[d + 1] < off[d]) return GFT_E_INVALID;
    for (uint64_t i = 0; i < n; i++)
        if (term[e0 + i] >= n_terms) return GFT_E_INVALID;
    uint64_t top = 0;
    if (n_docs) {
        const bool distinct = flags & GFT_SCORE_DISTINCT;
        const uint64_t G = stats_grid(n, n_docs, kHostResident);
        std::vector<uint64_t> set(kStatsSetSlots);
        std::vector<uint32_t> bits(distinct && !stats_bitset_in_lds(n_terms) ? stats_bitset_words(n_terms) : 0);
        for (uint64_t w = 0; w < G; w++) score_group(off, term, n_docs, n_terms, weights, distinct, w, G, score, top, set, bits);
    }
    if (max_score) *max_score = top;
    return GFT_OK;
}

int top_docs_host(const uint64_t* score, uint64_t n_docs, uint32_t k, uint64_t doc_base, uint64_t* top_idx, uint64_t* top_score, uint64_t* n_top) {
    if (n_top) *n_top = 0;
    if (k > kRankMaxK) return GFT_E_INVALID;
    if ((n_docs && !score) || (k && (!top_idx || !top_score))) return GFT_E_INVALID;
    if (n_docs > (~0ull >> 4)) return GFT_E_INVALID;
    if (top_buffers_overlap(score, n_docs, k, top_idx, top_score)) return GFT_E_INVALID;
    if (!k || !n_docs) return GFT_OK;
    // k_top_max
    uint64_t mx = 0;
    for (uint64_t d = 0; d < n_docs; d++) mx = std::max(mx, score[d]);
    if (!mx) return GFT_OK;
    // the select: k_top_hist, k_top_pick per digit
    uint64_t prefix = 0, krem = k;
    if (n_docs >= k)
        for (uint32_t p = rank_passes(mx); p--;) {
            const uint32_t shift = p * kRankDigitBits;
            std::vector<uint64_t> hist(kRankBins);
            for (uint64_t d = 0; d < n_docs; d++)
                if (rank_in_prefix(score[d], prefix, shift)) hist[rank_digit(score[d], shift)]++;
            uint64_t incl = 0;
            for (uint32_t lane = 0; lane < 64; lane++) {
                uint64_t cnt[kRankPickBins], mine = 0;
                for (uint32_t j = 0; j < kRankPickBins; j++) { cnt[j] = hist[rank_pick_bin(lane, j)]; mine += cnt[j]; }
                const uint64_t above = incl;
                incl += mine;
                if (above < krem && krem <= incl) {
                    prefix |= (uint64_t)rank_pick_in_lane(cnt, lane, above, krem) << shift;
                    break;
                }
            }
        }
    const uint64_t T = prefix;
    // k_top_count and the two prefix sums
    const uint64_t n_tiles = (n_docs + kRankPlaceTile - 1) / kRankPlaceTile;
    std::vector<uint64_t> gt_pos(n_tiles + 1), eq_pos(n_tiles + 1);
    for (uint64_t tile = 0; tile < n_tiles; tile++) {
        uint64_t gt = 0, eq = 0;
        for (uint32_t j = 0; j < kRankPlaceTrips; j++)
            for (uint32_t tid = 0; tid < kRankBlock; tid++) {
                const uint64_t d = rank_place_doc(tile, j, tid);
                const uint32_t cls = d < n_docs ? rank_class(score[d], T) : 0u;
                gt += cls == 2u; eq += cls == 1u;
            }
        gt_pos[tile + 1] = gt_pos[tile] + gt;
        eq_pos[tile + 1] = eq_pos[tile] + eq;
    }
    // k_top_place: a tile's rows of 64 documents, (trip, wave) in index order
    const uint64_t c = gt_pos[n_tiles], keep = rank_equals_kept(k, c, eq_pos[n_tiles]);
    std::vector<uint64_t> cand_score(k), cand_idx(k);
    for (uint64_t tile = 0; tile < n_tiles; tile++) {
        if (gt_pos[tile + 1] == gt_pos[tile] && (eq_pos[tile + 1] == eq_pos[tile] || eq_pos[tile] >= keep)) continue;
        uint32_t row_gt[kRankPlaceRows] = {0}, row_eq[kRankPlaceRows] = {0};
        for (uint32_t j = 0; j < kRankPlaceTrips; j++)
            for (uint32_t tid = 0; tid < kRankBlock; tid++) {
                const uint64_t d = rank_place_doc(tile, j, tid);
                const uint32_t cls = d < n_docs ? rank_class(score[d], T) : 0u;
                row_gt[rank_place_row(j, tid >> 6)] += cls == 2u;
                row_eq[rank_place_row(j, tid >> 6)] += cls == 1u;
            }
        for (uint32_t j = 0; j < kRankPlaceTrips; j++) {
            uint32_t in_gt = 0, in_eq = 0;                          // the lanes in front of this one in its row
            for (uint32_t tid = 0; tid < kRankBlock; tid++) {
                if ((tid & 63u) == 0) in_gt = in_eq = 0;
                const uint64_t d = rank_place_doc(tile, j, tid);
                const uint32_t cls = d < n_docs ? rank_class(score[d], T) : 0u;
                if (!cls) continue;
                const uint32_t row = rank_place_row(j, tid >> 6);
                uint64_t r = cls == 2u ? gt_pos[tile] : eq_pos[tile];
                for (uint32_t q = 0; q < row; q++) r += cls == 2u ? row_gt[q] : row_eq[q];
                r += cls == 2u ? in_gt++ : in_eq++;
                if (cls == 1u && r >= keep) continue;
                const uint64_t slot = cls == 2u ? r : c + r;
                if (slot >= k) continue;
                cand_score[slot] = score[d];
                cand_idx[slot] = d;
            }
        }
    }
    // k_top_sort
    const uint64_t listed = c + keep;
    const uint32_t n = listed < k ? (uint32_t)listed : k, N = rank_sort_size(n);
    std::vector<uint64_t> s_score(N), s_idx(N);
    for (uint32_t i = 0; i < N; i++) { s_score[i] = i < n ? cand_score[i] : 0; s_idx[i] = i < n ? cand_idx[i] : ~0ull; }
    for (uint32_t kk = 2; kk <= N; kk <<= 1)
        for (uint32_t j = kk >> 1; j; j >>= 1)
            for (uint32_t i = 0; i < N; i++) {
                uint32_t o;
                bool up;
                if (!rank_sort_pair(i, j, kk, o, up)) continue;
                if (up ? rank_before(s_score[o], s_idx[o], s_score[i], s_idx[i]) : rank_before(s_score[i], s_idx[i], s_score[o], s_idx[o])) {
                    std::swap(s_score[i], s_score[o]);
                    std::swap(s_idx[i], s_idx[o]);
                }
            }
    for (uint32_t i = 0; i < n; i++) { top_idx[i] = doc_base + s_idx[i]; top_score[i] = s_score[i]; }
    if (n_top) *n_top = n;
    return GFT_OK;
}

int gather_docs_host(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const uint64_t* idx, uint64_t m, uint64_t idx_base, uint8_t* out,
                     uint64_t cap_bytes, uint64_t* out_off, uint64_t* total_bytes) {
    if (total_bytes) *total_bytes = 0;
    if (!out_off || (m && !idx) || (n_docs && (!doc_off || !blob))) return GFT_E_INVALID;
    if (cap_bytes && !out) return GFT_E_INVALID;
    if (m > (~0ull >> 4) || n_docs > (~0ull >> 4)) return GFT_E_INVALID;
    if (m && !n_docs) return GFT_E_INVALID;
    if (!m) {
        if (ranges_meet(ByteRange{out_off, 8}, ByteRange{doc_off, (n_docs + 1) * 8})) return GFT_E_INVALID;
        out_off[0] = 0;
        return GFT_OK;
    }
    // k_gather_place and the prefix sum
    std::vector<uint64_t> c_off(m + 1), c_src(m);
    for (uint64_t j = 0; j < m; j++) {
        uint64_t d;
        if (!rank_gather_doc(idx[j], idx_base, n_docs, d) || !sel_doc_ok(doc_off[d], doc_off[d + 1])) return GFT_E_INVALID;
        c_src[j] = doc_off[d];
        c_off[j + 1] = c_off[j] + (doc_off[d + 1] - doc_off[d]);
    }
    const uint64_t total = c_off[m];
    if (gather_buffers_overlap(blob, doc_off[0], doc_off[n_docs], doc_off, n_docs, idx, m, out, cap_bytes, out_off)) return GFT_E_INVALID;
    if (total_bytes) *total_bytes = total;
    for (uint64_t j = 0; j <= m; j++) out_off[j] = c_off[j];
    select_copy_host(blob, c_off.data(), c_src.data(), m, sel_geom(total, cap_bytes, out), out);
    return GFT_OK;
}

}  // namespace gft
