// split_host.cpp -- gft_split_lines_device's walk on the host (gft_split.hpp): the count pass, the carry pass, the prefix sum and
// the write pass of gft_split.hip, tile by tile, trip by trip and lane by lane through gft_split_piece.hpp, with the ballots as
// loops.  Product code: the group finder's JSON Lines call splits with it when the finder does not take the device route.
#include <vector>

#include "../../include/gft.h"
#include "gft_split.hpp"

namespace gft {

namespace {

// one trip of a wave: the sixty-four pieces at tile * kSplitTile + t * kSplitTrip
struct Trip {
    uint64_t o[64];
    uint32_t nl[64], nw[64], flags[64];
    uint64_t NL = 0, HEAD = 0, TAIL = 0;
    Trip(const uint8_t* blob, uint64_t len, uint64_t tile, uint32_t t, bool after_nl) {
        for (uint32_t lane = 0; lane < 64; lane++) {
            o[lane] = tile * kSplitTile + t * kSplitTrip + lane * kSplitPiece;
            const uint32_t n = o[lane] < len ? (uint32_t)(len - o[lane] < kSplitPiece ? len - o[lane] : kSplitPiece) : 0u;
            uint32_t w[4] = {0, 0, 0, 0};
            if (n) split_load_piece(blob + o[lane], n, w);
            split_piece_masks(w, after_nl ? split_nl_bytes(o[lane], len) : n, nl[lane], nw[lane]);
            flags[lane] = split_piece_flags(nl[lane], nw[lane]);
            if (flags[lane] & kSplitHasNl) NL |= 1ull << lane;
            if (flags[lane] & kSplitHead) HEAD |= 1ull << lane;
            if (flags[lane] & kSplitTail) TAIL |= 1ull << lane;
        }
    }
    uint64_t last_nl(int lane) const { return o[lane] + (31u - (uint32_t)__builtin_clz(nl[lane])); }
    SplitSum sum(uint32_t count) const {
        int last;
        SplitSum s;
        s.flags = split_wave_flags(NL, HEAD, TAIL, &last);
        s.count = count;
        s.last_nl = last >= 0 ? last_nl(last) : 0;
        return s;
    }
};

}  // namespace

int split_lines_host(const uint8_t* blob, uint64_t len, uint32_t mode, uint64_t* doc_off, uint64_t cap, uint64_t* n_docs) {
    if (mode != GFT_SPLIT_AFTER_NL && mode != GFT_SPLIT_JSON_LINES) return GFT_E_INVALID;
    if (!n_docs || (len && !blob) || (cap && !doc_off)) return GFT_E_INVALID;
    *n_docs = 0;
    if (!len) {
        if (cap) doc_off[0] = 0;
        return GFT_OK;
    }
    const bool after_nl = mode == GFT_SPLIT_AFTER_NL;
    const uint64_t n_tiles = split_tiles(len);
    std::vector<uint32_t> cnt(n_tiles, 0);
    std::vector<uint64_t> base(n_tiles + 1, 0);
    std::vector<SplitSum> sums;
    std::vector<SplitCarry> carry;
    // k_split_count
    if (!after_nl) sums.assign(n_tiles, SplitSum{0, 0, 0});
    for (uint64_t tile = 0; tile < n_tiles; tile++) {
        SplitSum S{0, 0, 0};
        for (uint32_t t = 0; t < kSplitTrips; t++) {
            const Trip T(blob, len, tile, t, after_nl);
            uint32_t c = 0;
            for (uint32_t lane = 0; lane < 64; lane++) {
                if (after_nl) { c += (uint32_t)__builtin_popcount(T.nl[lane]); continue; }
                const SplitFrom F = split_lane_prefix(T.NL, T.HEAD, T.TAIL, lane, 0);
                c += (uint32_t)__builtin_popcount(split_inner_events(T.nl[lane], T.nw[lane])) +
                     ((F.src >= 0 && (T.flags[lane] & kSplitHead) && !F.open) ? 1u : 0u);
            }
            if (after_nl) cnt[tile] += c;
            else S = split_combine(S, T.sum(c));
        }
        if (!after_nl) sums[tile] = S;
    }
    // k_split_carry
    if (!after_nl) {
        carry.assign(n_tiles, SplitCarry{0, 0, 0});
        SplitCarry trip_carry{0, 0, 0};
        constexpr uint32_t kWaves = kSplitCarryBlock / 64;
        std::vector<SplitSum> run(kSplitCarryBlock);
        for (uint64_t t0 = 0; t0 < n_tiles; t0 += kSplitCarryTrip) {
            auto tile_sum = [&](uint64_t i) { return i < n_tiles ? sums[i] : SplitSum{0, 0, 0}; };
            uint64_t NL[kWaves] = {}, HEAD[kWaves] = {}, TAIL[kWaves] = {};
            SplitSum wave_sum[kWaves];
            for (uint32_t th = 0; th < kSplitCarryBlock; th++) {
                run[th] = SplitSum{0, 0, 0};
                for (uint32_t i = 0; i < kSplitCarryRun; i++) run[th] = split_combine(run[th], tile_sum(t0 + (uint64_t)th * kSplitCarryRun + i));
                if (run[th].flags & kSplitHasNl) NL[th >> 6] |= 1ull << (th & 63);
                if (run[th].flags & kSplitHead) HEAD[th >> 6] |= 1ull << (th & 63);
                if (run[th].flags & kSplitTail) TAIL[th >> 6] |= 1ull << (th & 63);
            }
            for (uint32_t w = 0; w < kWaves; w++) {
                int last;
                wave_sum[w].flags = split_wave_flags(NL[w], HEAD[w], TAIL[w], &last);
                wave_sum[w].count = 0;
                wave_sum[w].last_nl = last >= 0 ? run[w * 64 + (uint32_t)last].last_nl : 0;
            }
            for (uint32_t w = 0; w < kWaves; w++) {
                const SplitCarry c = trip_carry;                          // in front of wave w's runs
                for (uint32_t lane = 0; lane < 64; lane++) {
                    const uint32_t th = w * 64 + lane;
                    const SplitFrom F = split_lane_prefix(NL[w], HEAD[w], TAIL[w], lane, c.open);
                    SplitCarry mine{F.src >= 0 ? run[w * 64 + (uint32_t)F.src].last_nl + 1 : c.line_start, F.open, 0};
                    for (uint32_t i = 0; i < kSplitCarryRun; i++) {
                        const uint64_t tile = t0 + (uint64_t)th * kSplitCarryRun + i;
                        if (tile >= n_tiles) break;
                        carry[tile] = mine;
                        cnt[tile] = sums[tile].count + split_boundary(mine, sums[tile]);
                        mine = split_advance(mine, sums[tile]);
                    }
                }
                trip_carry = split_advance(trip_carry, wave_sum[w]);
            }
        }
    }
    // the prefix sum
    for (uint64_t tile = 0; tile < n_tiles; tile++) base[tile + 1] = base[tile] + cnt[tile];
    const uint64_t n = base[n_tiles] + (after_nl ? 1u : 0u);
    *n_docs = n;
    if (!cap) return GFT_OK;
    // k_split_write
    doc_off[0] = 0;
    if (n && n < cap) doc_off[n] = len;
    for (uint64_t tile = 0; tile < n_tiles; tile++) {
        uint64_t k = base[tile] + (after_nl ? 1u : 0u);
        SplitCarry c = after_nl ? SplitCarry{0, 0, 0} : carry[tile];
        for (uint32_t t = 0; t < kSplitTrips; t++) {
            const Trip T(blob, len, tile, t, after_nl);
            for (uint32_t lane = 0; lane < 64; lane++) {
                if (after_nl) {
                    split_emit_after_nl(T.nl[lane], T.o[lane], k, doc_off, cap);
                    k += (uint32_t)__builtin_popcount(T.nl[lane]);
                    continue;
                }
                const SplitFrom F = split_lane_prefix(T.NL, T.HEAD, T.TAIL, lane, c.open);
                const uint64_t line_start = F.src >= 0 ? T.last_nl(F.src) + 1 : c.line_start;
                uint32_t ev = split_inner_events(T.nl[lane], T.nw[lane]);
                if ((T.flags[lane] & kSplitHead) && !F.open) ev |= T.nw[lane] & (0u - T.nw[lane]);
                split_emit_lines(ev, T.nl[lane], T.o[lane], line_start, k, doc_off, cap);
                k += (uint32_t)__builtin_popcount(ev);
            }
            if (!after_nl) c = split_advance(c, T.sum(0));
        }
    }
    return GFT_OK;
}

}  // namespace gft
