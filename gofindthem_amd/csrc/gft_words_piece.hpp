// gft_words_piece.hpp -- whole-word matching (gft_filter_word_matches_device): what an entry of a match or span list decides,
// shared by the kernels (gft_words.hip) and the host walk (words_host.cpp).
//
// The rule.  A rune is a WORD rune when its general category starts with L, M or N, or is Pc (unicode_word.inc; U+FFFD and every
// byte the decoder rejects are not).  An occurrence is the bytes [s, e) of document D.  It is KEPT iff
//   NOT( word(utf8.DecodeLastRune(D[:s])) AND word(utf8.DecodeRune(D[s:e])) )   and
//   NOT( word(utf8.DecodeLastRune(D[s:e])) AND word(utf8.DecodeRune(D[e:])) ),
// with Go's strict decoder: overlong forms, surrogates and values above U+10FFFF are one RuneError each; DecodeLastRune goes back
// over at most UTFMax - 1 bytes to a rune start and answers RuneError unless the rune decoded there ends exactly at the slice's
// end; an empty slice has no rune and demands nothing.  RuneError is no word rune, so both decoders are needed only as "a valid
// sequence of a word rune begins at the slice's first byte / ends at its last", and neither ever reads a byte outside its slice:
// not the lead bytes, not the slack, not the neighbouring document, not the other half of a rune that a document border cuts.
//
// The walk.  keep[i] per entry, tile by tile of kWordsTile entries (a lane an entry) -> exclusive prefix sum rank -> entry rank[i]
// of the output = entry i, out_off[d] = rank[off[d] - off[0]]: a stable compaction, as the hit spans' (gft_spans_piece.hpp).
// Every text byte is read on its own (the four bytes round the two edges first: when all of them are ASCII nothing else is).
#pragma once
#include <stdint.h>

#ifndef GFT_HD
#if defined(__HIPCC__)
#define GFT_HD __host__ __device__
#else
#define GFT_HD
#endif
#endif

#include "gft_tolower_piece.hpp"

namespace gft {

constexpr uint32_t kWordsTile = 256;       // entries a workgroup of the check, mark and place passes takes per step
constexpr uint32_t kWordBlocks = 0x1100;   // 256-code-point blocks below 0x110000

// the check pass's flag words
constexpr uint32_t kWordsCtlOffs = 0;      // an offset descends
constexpr uint32_t kWordsCtlTerms = 1;     // a term id that is no index of the term table
constexpr uint32_t kWordsCtlRange = 2;     // an entry that leaves its document
constexpr uint32_t kWordsCtlWords = 4;

// The class table, two stages: row[cp >> 8] = the row of the block, bits[row * 8 + ((cp & 255) >> 5)] bit (cp & 31)
struct WordTable {
    const uint16_t* row;       // [kWordBlocks]
    const uint32_t* bits;      // [rows * 8]
};

GFT_HD inline uint32_t words_ascii_word(uint32_t b) {
    return ((b | 0x20u) - 'a' < 26u || b - '0' < 10u || b == '_') ? 1u : 0u;
}

// 1 or 0 for every value: 0 above U+10FFFF (surrogates and U+FFFD are 0 in the table)
GFT_HD inline uint32_t words_is_word(const WordTable& T, uint32_t cp) {
    if (cp < 0x80u) return words_ascii_word(cp);
    if (cp > 0x10FFFFu) return 0u;
    return T.bits[(uint32_t)T.row[cp >> 8] * 8u + ((cp & 255u) >> 5)] >> (cp & 31u) & 1u;
}

// word(utf8.DecodeRune(p[0 .. n))): 0 for an empty slice, for a byte that starts no valid sequence inside the slice, for a rune
// that is no word rune.  Reads p[0 .. min(n, 4)) at most.
GFT_HD inline uint32_t words_first_is_word(const WordTable& T, const uint8_t* p, uint64_t n) {
    if (!n) return 0u;
    const uint32_t b0 = p[0];
    if (b0 < 0x80u) return words_ascii_word(b0);
    if (b0 < 0xC2u || b0 > 0xF4u) return 0u;
    const uint32_t need = b0 < 0xE0u ? 2u : b0 < 0xF0u ? 3u : 4u;
    if (n < need) return 0u;
    const uint32_t b1 = p[1], b2 = need > 2 ? p[2] : 0u, b3 = need > 3 ? p[3] : 0u;
    uint32_t cp = 0;
    return tolower_decode(b0, b1, b2, b3, cp) ? words_is_word(T, cp) : 0u;
}

// word(utf8.DecodeLastRune(p[0 .. n))): the rune start is looked for among the three bytes in front of the last one, inside the
// slice; the sequence decoded there must end at the slice's end.  Reads p[max(n, 4) - 4 .. n) at most.
GFT_HD inline uint32_t words_last_is_word(const WordTable& T, const uint8_t* p, uint64_t n) {
    if (!n) return 0u;
    const uint32_t last = p[n - 1];
    if (last < 0x80u) return words_ascii_word(last);
    if (last >= 0xC0u) return 0u;                                  // a lead byte ends no sequence
    const uint32_t back = n < 4 ? (uint32_t)n - 1u : 3u;           // bytes of the slice in front of the last one, at most UTFMax - 1
    for (uint32_t k = 1; k <= back; k++) {
        const uint32_t b = p[n - 1 - k];
        if ((b & 0xC0u) == 0x80u) continue;                        // (no rune start: utf8.RuneStart)
        // the first rune start: Go decodes there and nowhere else
        if (b < 0xC2u || b > 0xF4u) return 0u;
        const uint32_t need = b < 0xE0u ? 2u : b < 0xF0u ? 3u : 4u;
        if (need != k + 1u) return 0u;                             // the sequence is cut short, or ends in front of the slice's end
        const uint8_t* q = p + (n - 1 - k);
        uint32_t cp = 0;
        return tolower_decode(b, q[1], need > 2 ? q[2] : 0u, need > 3 ? q[3] : 0u, cp) ? words_is_word(T, cp) : 0u;
    }
    return 0u;
}

// The two decoders once more for a walk that steps over the rune it judged (the excerpt's word snap, gft_excerpt_piece.hpp): the
// SIZE of the word rune that begins at the slice's first byte / ends at its last, 0 where words_first_is_word /
// words_last_is_word answer 0.  The same statements and the same reads.
GFT_HD inline uint32_t words_first_word_size(const WordTable& T, const uint8_t* p, uint64_t n) {
    if (!n) return 0u;
    const uint32_t b0 = p[0];
    if (b0 < 0x80u) return words_ascii_word(b0);
    if (b0 < 0xC2u || b0 > 0xF4u) return 0u;
    const uint32_t need = b0 < 0xE0u ? 2u : b0 < 0xF0u ? 3u : 4u;
    if (n < need) return 0u;
    const uint32_t b1 = p[1], b2 = need > 2 ? p[2] : 0u, b3 = need > 3 ? p[3] : 0u;
    uint32_t cp = 0;
    return (tolower_decode(b0, b1, b2, b3, cp) && words_is_word(T, cp)) ? need : 0u;
}
GFT_HD inline uint32_t words_last_word_size(const WordTable& T, const uint8_t* p, uint64_t n) {
    if (!n) return 0u;
    const uint32_t last = p[n - 1];
    if (last < 0x80u) return words_ascii_word(last);
    if (last >= 0xC0u) return 0u;
    const uint32_t back = n < 4 ? (uint32_t)n - 1u : 3u;
    for (uint32_t k = 1; k <= back; k++) {
        const uint32_t b = p[n - 1 - k];
        if ((b & 0xC0u) == 0x80u) continue;
        if (b < 0xC2u || b > 0xF4u) return 0u;
        const uint32_t need = b < 0xE0u ? 2u : b < 0xF0u ? 3u : 4u;
        if (need != k + 1u) return 0u;
        const uint8_t* q = p + (n - 1 - k);
        uint32_t cp = 0;
        return (tolower_decode(b, q[1], need > 2 ? q[2] : 0u, need > 3 ? q[3] : 0u, cp) && words_is_word(T, cp)) ? need : 0u;
    }
    return 0u;
}

// the occurrence [s, e) of the document doc[0 .. n): 1 when it is kept (s <= e <= n: the check pass saw to that)
GFT_HD inline uint32_t words_kept(const WordTable& T, const uint8_t* doc, uint64_t n, uint64_t s, uint64_t e) {
    if (s == e) return 1u;
    // the ASCII fast path: the four bytes at s - 1, s, e - 1 and e, all of them in the document and below 0x80
    if (s > 0 && e < n) {
        const uint32_t a = doc[s - 1], b = doc[s], c = doc[e - 1], d = doc[e];
        if (((a | b | c | d) & 0x80u) == 0)
            return ((words_ascii_word(a) & words_ascii_word(b)) | (words_ascii_word(c) & words_ascii_word(d))) ^ 1u;
    }
    if (words_last_is_word(T, doc, s) && words_first_is_word(T, doc + s, e - s)) return 0u;
    if (words_last_is_word(T, doc + s, e - s) && words_first_is_word(T, doc + e, n - e)) return 0u;
    return 1u;
}

// ---- the entries ----------------------------------------------------------------------------------------------------------
// where an entry of `len` bytes reported at `pos` begins (pos: its first byte, with pos_end its last); 0 when it would begin in
// front of its document (ok = 0).  An entry of length 0 reported at its "last byte" pos begins at pos + 1.
GFT_HD inline uint64_t words_entry_start(uint32_t pos, uint32_t len, uint32_t pos_end, uint32_t& ok) {
    ok = 1u;
    if (!pos_end) return pos;
    if ((uint64_t)pos + 1u < (uint64_t)len) { ok = 0u; return 0; }
    return (uint64_t)pos + 1u - len;
}

// entry (start, len) of the document [a, b) of the text: 1 when the document is one (offsets ascend) and the entry lies inside it
GFT_HD inline uint32_t words_entry_ok(uint64_t a, uint64_t b, uint64_t start, uint32_t len) {
    return (b >= a && start + (uint64_t)len <= b - a) ? 1u : 0u;
}

// the document of entry m: the d < n_docs with off[d] <= m < off[d + 1] (off[0] <= m < off[n_docs]; n_docs >= 1).  Ends inside
// [0, n_docs) whatever the offsets hold.
GFT_HD inline uint64_t words_doc_of(const uint64_t* off, uint64_t n_docs, uint64_t m) {
    uint64_t lo = 0, hi = n_docs - 1;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (off[mid + 1] <= m) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

}  // namespace gft
