// words_host.cpp -- the walk of gft_words.hip on the host (gft_words.hpp): the check pass, then mark, prefix sum and place, entry
// tile by entry tile through gft_words_piece.hpp, the search and the decoders included; and the class table of unicode_word.inc.
// No device, no handle.
#include <algorithm>
#include <vector>

#include "../../include/gft.h"
#include "gft_words.hpp"

namespace gft {

namespace {
#include "unicode_word.inc"
const WordTable kHostTable{kWordBlockRow, kWordRowBits};
static_assert(sizeof kWordBlockRow / sizeof kWordBlockRow[0] == kWordBlocks, "one row index per block of 256 code points");
static_assert(sizeof kWordRowBits / sizeof kWordRowBits[0] == GFT_WORD_ROWS * 8u, "rows of 256 bits");
}  // namespace

const WordTable& word_table_host() { return kHostTable; }
uint32_t word_table_rows() { return GFT_WORD_ROWS; }

int filter_word_matches_host(const uint8_t* text, const uint64_t* doc_off, uint64_t n_docs, const uint64_t* off, const uint32_t* pos,
                             const uint32_t* len, const uint32_t* term, const uint32_t* term_len, uint32_t n_terms, uint32_t flags,
                             uint64_t* out_off, uint32_t* out_pos, uint32_t* out_len, uint32_t* out_term, uint64_t cap, uint64_t* total) {
    if (total) *total = 0;
    if (flags & ~GFT_WORDS_POS_END) return GFT_E_INVALID;
    if (cap && !out_pos) return GFT_E_INVALID;
    if (!n_docs) {
        if (out_off) out_off[0] = 0;
        return GFT_OK;
    }
    if (!doc_off || !off) return GFT_E_INVALID;
    if (off[n_docs] < off[0]) return GFT_E_INVALID;
    const uint64_t e0 = off[0], n = off[n_docs] - e0;
    if (n && (!text || !pos || (!len && (!term || !term_len)) || (out_term && !term))) return GFT_E_INVALID;
    const uint32_t pos_end = (flags & GFT_WORDS_POS_END) ? 1u : 0u;
    {
        uint64_t lo = doc_off[0], hi = doc_off[0];
        for (uint64_t d = 0; d <= n_docs; d++) { lo = std::min(lo, doc_off[d]); hi = std::max(hi, doc_off[d]); }
        const ByteRange ins[7] = {{text ? text + lo : nullptr, hi - lo}, {doc_off, (n_docs + 1) * 8}, {off, (n_docs + 1) * 8},
                                  {pos ? pos + e0 : nullptr, n * 4}, {len ? len + e0 : nullptr, n * 4}, {term ? term + e0 : nullptr, n * 4},
                                  {len ? nullptr : term_len, (uint64_t)n_terms * 4}};
        if (words_outputs_overlap(out_off, n_docs, out_pos, out_len, out_term, cap, ins, 7)) return GFT_E_INVALID;
    }
    // k_words_check
    bool bad = false;
    for (uint64_t d = 0; d < n_docs; d++) bad |= off[d + 1] < off[d];
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t m = e0 + i;
        uint32_t L;
        if (len) {
            L = len[m];
        } else {
            if (term[m] >= n_terms) { bad = true; continue; }
            L = term_len[term[m]];
        }
        const uint64_t d = words_doc_of(off, n_docs, m);
        uint32_t ok;
        const uint64_t start = words_entry_start(pos[m], L, pos_end, ok);
        if (!ok || !words_entry_ok(doc_off[d], doc_off[d + 1], start, L)) bad = true;
    }
    if (bad) return GFT_E_INVALID;
    // k_words_mark, a workgroup's tile at a time
    const WordTable& T = word_table_host();
    std::vector<uint32_t> keep(n);
    for (uint64_t i0 = 0; i0 < n; i0 += kWordsTile)
        for (uint64_t i = i0; i < std::min<uint64_t>(i0 + kWordsTile, n); i++) {
            const uint64_t m = e0 + i;
            const uint32_t L = len ? len[m] : term_len[term[m]];
            const uint64_t d = words_doc_of(off, n_docs, m);
            const uint64_t a = doc_off[d], b = doc_off[d + 1];
            uint32_t ok;
            const uint64_t start = words_entry_start(pos[m], L, pos_end, ok);
            keep[i] = words_kept(T, text + a, b - a, start, start + L);
        }
    // the prefix sum
    std::vector<uint64_t> rank(n + 1, 0);
    for (uint64_t i = 0; i < n; i++) rank[i + 1] = rank[i] + keep[i];
    if (total) *total = rank[n];
    // k_words_place
    for (uint64_t i = 0; i < std::max(n_docs + 1, n); i++) {
        if (out_off && i <= n_docs) out_off[i] = rank[off[i] - e0];
        if (i >= n || !keep[i]) continue;
        const uint64_t r = rank[i];
        if (r >= cap) continue;
        const uint64_t m = e0 + i;
        out_pos[r] = pos[m];
        if (out_len) out_len[r] = len ? len[m] : term_len[term[m]];
        if (out_term) out_term[r] = term[m];
    }
    return GFT_OK;
}

}  // namespace gft
