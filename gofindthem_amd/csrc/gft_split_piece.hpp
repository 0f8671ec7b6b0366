// gft_split_piece.hpp -- a resident blob cut into line documents (gft_split_lines_device): what a 16-byte piece, a wave's trip, a
// tile and a carry say, shared by the kernels (gft_split.hip) and the host walk (split_host.cpp).
//
// GFT_SPLIT_AFTER_NL: a document starts behind every '\n' that is not the blob's last byte -- a count of newlines, no carry.
// GFT_SPLIT_JSON_LINES: a document starts where a non-blank line starts; the event sits at the line's first byte that is not JSON
// whitespace (20 09 0A 0D), the value written is the line's start.  Whether a byte is the first of its line depends on
// everything back to the previous newline, so a stretch of text is summarised by a SplitSum:
//
//   has_nl    it holds a newline                     last_nl   the position of its last one
//   head      a non-whitespace byte in front of its first newline (anywhere, when it holds none; tail is then the same bit)
//   tail      a non-whitespace byte behind its last newline
//   count     the documents that start inside it whatever lies in front: first bytes of lines that begin behind one of ITS newlines
//
// split_combine(a, b) is the summary of a followed by b: associative, the empty summary is its identity.  What lies in front of
// a stretch is a SplitCarry -- where the open line began and whether it already has a non-whitespace byte --; the stretch's
// head then starts one more document (split_boundary) exactly when the carry's line is still blank.
#pragma once
#include <stdint.h>
#include <string.h>

#ifndef GFT_HD
#if defined(__HIPCC__)
#define GFT_HD __host__ __device__
#else
#define GFT_HD
#endif
#endif

namespace gft {

constexpr uint32_t kSplitPiece = 16;                         // bytes per lane and trip: one 16-byte load
constexpr uint32_t kSplitTrip = 64 * kSplitPiece;            // bytes per wave and trip
constexpr uint32_t kSplitTrips = 4;                          // trips per tile, their loads issued together
constexpr uint32_t kSplitTile = kSplitTrips * kSplitTrip;    // a wave's contiguous run: 4 KiB
constexpr uint32_t kSplitCarryBlock = 256;                   // the carry kernel: one workgroup, ...
constexpr uint32_t kSplitCarryRun = 4;                       // ... consecutive tiles per thread, ...
constexpr uint32_t kSplitCarryTrip = kSplitCarryBlock * kSplitCarryRun;   // ... tiles per trip of it

enum : uint32_t { kSplitHasNl = 1, kSplitHead = 2, kSplitTail = 4 };

struct SplitSum {
    uint64_t last_nl;
    uint32_t flags, count;
};
struct SplitCarry {
    uint64_t line_start;
    uint32_t open, pad;
};

// 0x80 in every byte of x that is zero (exact: no borrow between bytes)
GFT_HD inline uint32_t split_zero4(uint32_t x) { return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu); }
// bits 7, 15, 23, 31 -> bits 0..3
GFT_HD inline uint32_t split_pack4(uint32_t m) { return ((m >> 7) * 0x01020408u) >> 24; }

// the piece's sixteen bytes as four words; n of them belong to the blob.  The device reads all sixteen (the blob is readable
// 64 bytes past its end), the host only its own.
GFT_HD inline void split_load_piece(const uint8_t* p, uint32_t n, uint32_t w[4]) {
#if defined(__HIP_DEVICE_COMPILE__)
    struct __attribute__((packed, aligned(1))) U128u { uint32_t x, y, z, w; };
    const U128u v = *reinterpret_cast<const U128u*>(p);
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    (void)n;
#else
    w[0] = w[1] = w[2] = w[3] = 0;
    memcpy(w, p, n < kSplitPiece ? n : kSplitPiece);
#endif
}

// bit i of nl: byte i is '\n'; of nw: byte i is not JSON whitespace; i < n
GFT_HD inline void split_piece_masks(const uint32_t w[4], uint32_t n, uint32_t& nl, uint32_t& nw) {
    nl = nw = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4; q++) {
        const uint32_t e_nl = split_zero4(w[q] ^ 0x0A0A0A0Au);
        const uint32_t ws = e_nl | split_zero4(w[q] ^ 0x20202020u) | split_zero4((w[q] & 0xFBFBFBFBu) ^ 0x09090909u);   // 09 and 0D
        nl |= split_pack4(e_nl) << (4 * q);
        nw |= split_pack4(~ws & 0x80808080u) << (4 * q);
    }
    const uint32_t valid = n >= kSplitPiece ? 0xFFFFu : (1u << n) - 1u;
    nl &= valid; nw &= valid;
}

// GFT_SPLIT_AFTER_NL: the newline that is the blob's last byte starts nothing -- the bytes of the piece at o that may
GFT_HD inline uint32_t split_nl_bytes(uint64_t o, uint64_t len) {
    return len > o + 1 ? (uint32_t)(len - 1 - o < kSplitPiece ? len - 1 - o : kSplitPiece) : 0u;
}

// first non-whitespace bytes of the lines that begin behind a newline of the piece: the carry of (nl << 1) runs through the
// bytes that are neither and stops at the next one that is either
GFT_HD inline uint32_t split_inner_events(uint32_t nl, uint32_t nw) {
    const uint32_t x = nl | nw;
    return ((nl << 1) + (~x & 0x1FFFFu)) & nw;
}

GFT_HD inline uint32_t split_piece_flags(uint32_t nl, uint32_t nw) {
    if (!nl) return nw ? (kSplitHead | kSplitTail) : 0u;
    const uint32_t first = (uint32_t)__builtin_ctz(nl), last = 31u - (uint32_t)__builtin_clz(nl);
    return kSplitHasNl | ((nw & ((1u << first) - 1u)) ? kSplitHead : 0u) | ((nw >> (last + 1)) ? kSplitTail : 0u);
}

// Sixty-four summaries side by side (the pieces of a trip, or the runs of the carry kernel) as three masks: NL, HEAD, TAIL = who
// has which flag.  What lane `lane` has in front of it: src = the nearest lane below it with a newline (-1: none, the line
// comes from the carry), open = that line already has a non-whitespace byte.
struct SplitFrom {
    int src;
    uint32_t open;
};
GFT_HD inline SplitFrom split_lane_prefix(uint64_t NL, uint64_t HEAD, uint64_t TAIL, uint32_t lane, uint32_t carry_open) {
    const uint64_t below = lane ? ~0ull >> (64 - lane) : 0ull;
    const uint64_t nlb = NL & below;
    if (!nlb) return SplitFrom{-1, carry_open | ((HEAD & below) ? 1u : 0u)};
    const int j = 63 - __builtin_clzll(nlb);                               // (j < lane <= 63)
    const uint64_t between = below & ~((2ull << j) - 1ull);
    return SplitFrom{j, (uint32_t)((TAIL >> j) & 1u) | ((HEAD & between) ? 1u : 0u)};
}
// the flags of the sixty-four together; *last = the highest lane with a newline, or -1
GFT_HD inline uint32_t split_wave_flags(uint64_t NL, uint64_t HEAD, uint64_t TAIL, int* last) {
    if (!NL) { *last = -1; return HEAD ? (kSplitHead | kSplitTail) : 0u; }
    const int f = __builtin_ctzll(NL), l = 63 - __builtin_clzll(NL);
    *last = l;
    const uint64_t upto = f == 63 ? ~0ull : (2ull << f) - 1ull;
    const bool tail = ((TAIL >> l) & 1u) || (l < 63 && (HEAD >> (l + 1)));
    return kSplitHasNl | ((HEAD & upto) ? kSplitHead : 0u) | (tail ? kSplitTail : 0u);
}

GFT_HD inline SplitSum split_combine(const SplitSum& a, const SplitSum& b) {
    const bool an = a.flags & kSplitHasNl, bn = b.flags & kSplitHasNl;
    const uint32_t any_b = (b.flags & kSplitHead) ? 1u : 0u;
    SplitSum r;
    r.count = a.count + b.count + ((an && any_b && !(a.flags & kSplitTail)) ? 1u : 0u);
    const uint32_t head = (a.flags & kSplitHead) || (!an && any_b);
    const uint32_t tail = bn ? (b.flags & kSplitTail) != 0 : ((a.flags & kSplitTail) || any_b);
    r.flags = ((an || bn) ? kSplitHasNl : 0u) | (head ? kSplitHead : 0u) | (tail ? kSplitTail : 0u);
    r.last_nl = bn ? b.last_nl : a.last_nl;
    return r;
}
// the document that s's head starts when c lies in front of it
GFT_HD inline uint32_t split_boundary(const SplitCarry& c, const SplitSum& s) { return ((s.flags & kSplitHead) && !c.open) ? 1u : 0u; }
// the carry behind s
GFT_HD inline SplitCarry split_advance(const SplitCarry& c, const SplitSum& s) {
    if (s.flags & kSplitHasNl) return SplitCarry{s.last_nl + 1, (s.flags & kSplitTail) ? 1u : 0u, 0u};
    return SplitCarry{c.line_start, c.open | ((s.flags & kSplitHead) ? 1u : 0u), 0u};
}

// Stores the starts of the piece at o: event bits ev (inner events, and the boundary event below the first newline, whose line
// began at carry_start) take the ranks k, k + 1, ..; rank 0 is the blob's start and is written elsewhere.  An entry at or past
// cap is not stored.
GFT_HD inline void split_emit_lines(uint32_t ev, uint32_t nl, uint64_t o, uint64_t carry_start, uint64_t k, uint64_t* out, uint64_t cap) {
    while (ev) {
        const uint32_t i = (uint32_t)__builtin_ctz(ev);
        ev &= ev - 1;
        const uint32_t before = nl & ((1u << i) - 1u);
        const uint64_t v = before ? o + (32u - (uint32_t)__builtin_clz(before)) : carry_start;
        if (k && k < cap) out[k] = v;
        k++;
    }
}
// GFT_SPLIT_AFTER_NL: the byte behind every newline of nl
GFT_HD inline void split_emit_after_nl(uint32_t nl, uint64_t o, uint64_t k, uint64_t* out, uint64_t cap) {
    while (nl) {
        const uint32_t i = (uint32_t)__builtin_ctz(nl);
        nl &= nl - 1;
        if (k < cap) out[k] = o + i + 1;
        k++;
    }
}

}  // namespace gft
