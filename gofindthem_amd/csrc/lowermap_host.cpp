// lowermap_host.cpp -- the walk of gft_map_spans_to_source_device on the host (gft_lowermap.hpp): the unit table, the count pass,
// the prefix sum and the table pass unit by unit, trip by trip and piece by piece as k_lower runs them, then the check and the
// write pass span tile by span tile -- all through gft_tolower_piece.hpp, gft_lowermap_piece.hpp and gft_spans_piece.hpp, the
// searches included.  No device, no handle.
#include <algorithm>
#include <vector>

#include "../../include/gft.h"
#include "gft_lowermap.hpp"

namespace gft {

int lowermap_host(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const uint64_t* span_off, uint32_t* span_start,
                  uint32_t* span_len, uint64_t limit) {
    if (!n_docs) return GFT_OK;
    if (!doc_off || !span_off || span_off[n_docs] < span_off[0]) return GFT_E_INVALID;
    const uint64_t s0 = span_off[0], n = std::min(span_off[n_docs], std::max(limit, s0)) - s0;
    if (!n) return GFT_OK;
    if (!blob || !span_start || !span_len) return GFT_E_INVALID;
    const LowerTable T = lower_table_host().view();
    std::vector<uint64_t> unit_base;
    std::vector<Unit> units;
    if (int rc = lower_units_host(doc_off, n_docs, unit_base, units)) return rc;
    // a unit's pieces in the kernel's order: trips of 64 pieces; piece(window, own bytes, index in the unit)
    auto walk = [&](const Unit& un, auto&& piece) {
        const uint64_t doc_abs = doc_off[un.doc], doc_len = doc_off[un.doc + 1] - doc_abs;
        for (uint64_t base = un.lo; base < un.hi; base += kLowerChunk)
            for (uint32_t lane = 0; lane < 64; lane++) {
                const uint64_t o = base + lane * kLowerPiece;
                if (o >= un.hi) break;
                LowerWin w;
                tolower_load_piece(blob + doc_abs + o, o < 3 ? (uint32_t)o : 3u, doc_len - o, w);
                piece(w, (uint32_t)std::min<uint64_t>(kLowerPiece, un.hi - o), (o - un.lo) / kLowerPiece);
            }
    };
    // k_lower<kLowerCount> and the prefix sum
    std::vector<uint64_t> unit_out(units.size() + 1, 0);
    for (size_t u = 0; u < units.size(); u++) {
        uint64_t cnt = 0;
        walk(units[u], [&](const LowerWin& w, uint32_t own, uint64_t) { cnt += tolower_piece<false>(T, w, own, nullptr, 0, 0); });
        unit_out[u + 1] = unit_out[u] + cnt;
    }
    for (uint64_t d = 0; d < n_docs; d++)
        if (unit_out[unit_base[d + 1]] - unit_out[unit_base[d]] > 0xFFFFFFFFull) return GFT_E_INVALID;
    // k_lower<kLowerTable>: slots that no piece owns keep a pattern that no search may read
    std::vector<uint32_t> tab(lowermap_slots(doc_off[n_docs] - doc_off[0], units.size()), 0xDEADBEEFu);
    for (size_t u = 0; u < units.size(); u++) {
        const Unit& un = units[u];
        uint64_t carry = unit_out[u] - unit_out[unit_base[un.doc]];
        const uint64_t slot = lowermap_slot(doc_off[un.doc] - doc_off[0] + un.lo, u);
        walk(un, [&](const LowerWin& w, uint32_t own, uint64_t j) {
            tab[slot + j] = (uint32_t)carry;
            carry += tolower_piece<false>(T, w, own, nullptr, 0, 0);
        });
    }
    const LowerMapView V{blob, doc_off, n_docs, unit_base.data(), units.data(), unit_out.data(), tab.data(), T};
    // k_lowermap_check, a wave's tile at a time
    std::vector<uint32_t> mapped(2 * n, 0);
    bool bad = false;
    for (uint64_t k0 = 0; k0 < n; k0 += kMapTile)
        for (uint64_t k = k0; k < std::min<uint64_t>(k0 + kMapTile, n); k++) {
            const uint64_t d = span_doc_of(span_off, n_docs, s0 + k);
            if (!lowermap_span(V, d, span_start[s0 + k], span_len[s0 + k], mapped[2 * k], mapped[2 * k + 1])) bad = true;
        }
    if (bad) return GFT_E_INVALID;
    // k_lowermap_write
    for (uint64_t k = 0; k < n; k++) {
        span_start[s0 + k] = mapped[2 * k];
        span_len[s0 + k] = mapped[2 * k + 1];
    }
    return GFT_OK;
}

}  // namespace gft
