// tolower_host.cpp -- the host side of the device's strings.ToLower: the two-level mapping table derived from the one
// array of (code point, lower-case form) pairs, and gft_to_lower_device's walk on the host through the kernel's own piece
// logic (gft_tolower_piece.hpp) -- what gft_debug_lower_rune / gft_debug_emulate_to_lower answer from.
#include "gft_tolower.hpp"

#include <algorithm>
#include <cstring>

#include "../../include/gft.h"
#include "dsl_compile.hpp"
#include "gft_guard.hpp"
#include "gft_overlap.hpp"

namespace gft {

const LowerTableHost& lower_table_host() {
    static const LowerTableHost table = [] {
        LowerTableHost t;
        size_t n = 0;
        const dsl::LowerPair* pairs = dsl::LowerPairs(&n);
        t.page.assign(n ? ((size_t)pairs[n - 1].from >> kLowerPageShift) + 1 : 0, 0);
        t.delta.assign(64, 0);
        for (size_t i = 0; i < n; i++) {
            if (pairs[i].from == pairs[i].to) continue;
            uint16_t& row = t.page[(size_t)pairs[i].from >> kLowerPageShift];
            if (!row) {
                row = (uint16_t)(t.delta.size() / 64);
                t.delta.resize(t.delta.size() + 64, 0);
            }
            t.delta[(size_t)row * 64 + (pairs[i].from & 63)] = pairs[i].to - pairs[i].from;
        }
        return t;
    }();
    return table;
}

bool lower_buffers_overlap(const uint8_t* text, uint64_t lo, uint64_t hi, const uint64_t* doc_off, uint64_t n_docs, const uint8_t* out,
                           uint64_t cap, const uint64_t* out_off) {
    const ByteRange outs[] = {{out, cap}, {out_off, (n_docs + 1) * 8}};
    // (the slack behind the text is read, but no byte of it decides anything)
    const ByteRange ins[] = {{text ? text + lo : nullptr, hi > lo ? hi - lo : 0}, {doc_off, (n_docs + 1) * 8}};
    return outputs_overlap(outs, ins);
}

// the unit table (k_unit_count, the prefix sum, k_unit_fill)
int lower_units_host(const uint64_t* doc_off, uint64_t n_docs, std::vector<uint64_t>& unit_base, std::vector<Unit>& units) {
    unit_base.assign(n_docs + 1, 0);
    for (uint64_t d = 0; d < n_docs; d++) {
        if (doc_off[d + 1] < doc_off[d] || doc_off[d + 1] - doc_off[d] > 0xFFFFFFFFull) return GFT_E_INVALID;
        const uint64_t n = doc_off[d + 1] - doc_off[d];
        unit_base[d + 1] = unit_base[d] + (n <= kLowerUnitMax ? 1 : (n + kLowerUnitMax - 1) / kLowerUnitMax);
    }
    units.resize(unit_base[n_docs]);
    for (uint64_t d = 0; d < n_docs; d++) {
        const uint64_t n = doc_off[d + 1] - doc_off[d], k = unit_base[d + 1] - unit_base[d], per = (n + k - 1) / k;
        for (uint64_t i = 0; i < k; i++) units[unit_base[d] + i] = Unit{(uint32_t)d, (uint32_t)std::min(i * per, n), (uint32_t)std::min(i * per + per, n)};
    }
    return GFT_OK;
}

int lower_emulate(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, uint8_t* out, uint64_t cap, uint64_t* out_off,
                  uint64_t* total) {
    const LowerTable T = lower_table_host().view();
    std::vector<uint64_t> unit_base;
    std::vector<Unit> units;
    if (int rc = lower_units_host(doc_off, n_docs, unit_base, units)) return rc;
    // a unit's pieces in the kernel's order: trips of 64 pieces
    auto walk = [&](const Unit& un, auto&& piece) {
        const uint64_t doc_abs = doc_off[un.doc], doc_len = doc_off[un.doc + 1] - doc_abs;
        for (uint64_t base = un.lo; base < un.hi; base += kLowerChunk)
            for (uint32_t lane = 0; lane < 64; lane++) {
                const uint64_t o = base + lane * kLowerPiece;
                if (o >= un.hi) break;
                LowerWin w;
                tolower_load_piece(blob + doc_abs + o, o < 3 ? (uint32_t)o : 3u, doc_len - o, w);
                piece(w, (uint32_t)std::min<uint64_t>(kLowerPiece, un.hi - o));
            }
    };
    std::vector<uint64_t> unit_out(units.size() + 1, 0);
    for (size_t u = 0; u < units.size(); u++) {
        uint64_t cnt = 0;
        walk(units[u], [&](const LowerWin& w, uint32_t n) { cnt += tolower_piece<false>(T, w, n, nullptr, 0, 0); });
        unit_out[u + 1] = unit_out[u] + cnt;
    }
    bool too_long = false;
    for (uint64_t d = 0; d <= n_docs; d++) {
        out_off[d] = unit_out[unit_base[d]];
        if (d && out_off[d] - out_off[d - 1] > 0xFFFFFFFFull) too_long = true;
    }
    if (total) *total = unit_out[units.size()];
    if (too_long) return GFT_E_INVALID;
    if (cap)
        for (size_t u = 0; u < units.size(); u++) {
            uint64_t pos = unit_out[u];
            walk(units[u], [&](const LowerWin& w, uint32_t n) { pos += tolower_piece<true>(T, w, n, out, pos, cap); });
        }
    return GFT_OK;
}

}  // namespace gft

extern "C" {

uint32_t gft_debug_lower_rune(uint32_t cp) try {
    return gft::tolower_rune(gft::lower_table_host().view(), cp);
} GFT_CATCH_VALUE(cp)

int gft_debug_emulate_to_lower(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, uint8_t* out, uint64_t cap, uint64_t* out_off,
                               uint64_t* total) try {
    if (!doc_off || !out_off || (cap && !out)) return GFT_E_INVALID;
    for (uint64_t d = 0; d < n_docs; d++)
        if (doc_off[d + 1] < doc_off[d] || doc_off[d + 1] - doc_off[d] > 0xFFFFFFFFull) return GFT_E_INVALID;
    if (doc_off[n_docs] > doc_off[0] && !blob) return GFT_E_INVALID;
    if (gft::lower_buffers_overlap(blob, doc_off[0], doc_off[n_docs], doc_off, n_docs, out, cap, out_off)) return GFT_E_INVALID;
    // (the pieces load up to 20 bytes from their first one: the walk runs on a copy with the slack the device entry asks
    // of its caller; offsets are rebased to it)
    const uint64_t lo = doc_off[0], len = doc_off[n_docs] - lo;
    std::vector<uint8_t> text((size_t)len + 64, 0);
    if (len) memcpy(text.data(), blob + lo, (size_t)len);
    std::vector<uint64_t> off(n_docs + 1);
    for (uint64_t d = 0; d <= n_docs; d++) off[d] = doc_off[d] - lo;
    return gft::lower_emulate(text.data(), off.data(), n_docs, out, cap, out_off, total);
} GFT_CATCH(nullptr)

}  // extern "C"
