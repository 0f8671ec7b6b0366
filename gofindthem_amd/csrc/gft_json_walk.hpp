// gft_json_walk.hpp -- the JSON walker of the group finder's device front (gft_json.hip), compiled for the device and for the
// host: the kernels and the host emulation (json_schema.cpp: json_leaves_emulate) run this one source.
//
// A wave owns a document and reads it in pieces of 64 bytes, a byte per lane.  Per piece, 64-bit masks say where the quotes,
// the backslashes, the whitespace and the bytes inside strings are (json_piece_masks): escaped characters come from the
// odd-backslash-run mask, the in-string mask is the prefix XOR of the quotes that are left, both carried from piece to
// piece.  The grammar and the schema trie are then walked wave-uniformly over the set bits of the event mask -- every byte
// that is neither whitespace nor inside a string --; string interiors are handled as lane masks (json_segment): checked,
// counted, and copied with a per-lane prefix count as the output position.
//
// What works on lanes comes through the policy class W, which the device fills with ballots and the host with loops:
//     load(doc, base, len)      the piece: lane l holds byte base + l of the document, 0 behind its end
//     lane_byte(l), byte_at(k)  a lane's own byte; byte k of the piece, wave-uniform
//     ballot(f), sum(f)         f(lane) over the 64 lanes -> mask / sum
//     each(f), once(f)          f(lane) in every lane; f() in one
//     out(l), flags(l)          JsonLaneOut and class bits of lane l, kept from json_piece_masks to json_segment
//     uni(x)                    x, which is the same in every lane (the device moves it to a scalar register)
//     mem()                     JsonWaveMem of the wave (LDS on the device)
//
// Three ways to run the walk, chosen at compile time by the policy class D (json_walk_doc):
//     JsonNoPaths     against the schema trie: count pass and write pass (json_walk_doc)
//     JsonPaths       discovery: no trie.  The wave remembers where it is -- per tracked container the member key that is open
//                     (JsonPathMem) -- and hands the path of every string value to a set of 64-bit path hashes
//                     (json_path_found); the wave that puts a hash in first writes the path's bytes into a pool.
// A path is spelled as getRulesInfo spells it (internal.go:46-47, 68-69, 82-84): components joined by '.', a key as its raw
// bytes, an array element as "index(<i>)", the root as "".  No path is produced below a key that raises kJsKey, below
// container depth 32, or when the path is longer than 65 535 bytes.  A value under a key that contains '.' IS reported, with
// the key's bytes as one component: the path then reads like that of a nested member, which is harmless -- such a key resolves
// to nothing in the trie, and the document ends as GFT_JSON_PATH on the host route (the two spellings of one path string hash
// differently; the host removes the duplicate).
//
// Statuses and the class of documents that is decided here: include/gft.h (gft_json_status).  A document is walked to its end
// also after a condition other than GFT_JSON_SYNTAX was met: every condition sets its bit, the lowest status wins, so that
// the answer does not depend on the order in which a walker meets them.  Nothing outside [0, len) of the document is read.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GFT_JHD __host__ __device__
#else
#define GFT_JHD
#endif

namespace gft {

constexpr uint32_t kJsonNone = 0xFFFFFFFFu;        // no node / no field
constexpr uint32_t kJsonMaxNodes = 16384;          // the visited bitset: 2 KB per wave
constexpr uint32_t kJsonMaxKey = 65535;            // bytes of one component
constexpr uint32_t kJsonMaxDepth = 32;             // containers open at once that the walker tracks
constexpr uint32_t kJsonHardDepth = 10000;         // ... that json_mini accepts (encoding/json's limit)

enum : uint32_t { kJsOk = 0, kJsSyntax = 1, kJsDepth = 2, kJsPath = 3, kJsKey = 4, kJsDup = 5, kJsText = 6 };

struct JsonTrieNode { uint32_t parent, key_off, key_len, field; };
struct JsonTrie {
    const JsonTrieNode* nodes; const uint8_t* keys; const uint32_t* table;
    uint32_t table_mask, n_nodes, max_key_len;
};

struct JsonWaveMem {
    uint32_t visited[kJsonMaxNodes / 32];          // trie nodes reached in this document
    uint32_t kinds[(kJsonHardDepth + 31) / 32];    // bit d: the container at depth d is an object
    uint32_t node[kJsonMaxDepth];                  // the trie node of the container at depth d, or kJsonNone
    uint32_t count[kJsonMaxDepth];                 // the index of the array element being read
};

struct JsonLaneOut { uint8_t n, o[3]; };           // what a byte inside a string becomes: 0..3 bytes

// where a document's leaves go (all NULL / 0 in the count pass)
struct JsonDocOut {
    uint32_t* leaf_field; uint64_t* leaf_off; uint8_t* text;
    uint64_t leaf_cap, text_cap, leaf_base, text_base;
};

// ---- hashing a component: a sum of per-byte terms, so that the lanes can add their shares in any order ---------------
GFT_JHD inline uint32_t json_key_term(uint32_t b, uint32_t j) {
    uint32_t t = (b + 1u) * 0x9E3779B1u;
    t ^= t >> 15;
    return t * (2u * j + 1u);
}
GFT_JHD inline uint32_t json_slot_hash(uint32_t parent, uint32_t h) {
    uint32_t x = h + parent * 0x85EBCA6Bu;
    x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15;
    return x;
}
struct JsonKeyMem {                                // a key's bytes in the document / a component given by the caller
    const uint8_t* p;
    GFT_JHD uint32_t operator()(uint32_t j) const { return p[j]; }
};
struct JsonKeyIndex {                              // "index(<i>)", the component of array element i (internal.go:84)
    uint32_t i, nd;
    GFT_JHD explicit JsonKeyIndex(uint32_t i_) : i(i_), nd(1) { for (uint32_t v = i_; v >= 10; v /= 10) nd++; }
    GFT_JHD uint32_t len() const { return 7 + nd; }
    GFT_JHD uint32_t operator()(uint32_t j) const {
        if (j < 6) return (uint32_t)((0x287865646E69ull >> (8 * j)) & 0xFF);    // "index("
        if (j >= 6 + nd) return ')';
        uint32_t v = i;
        for (uint32_t s = 6 + nd - 1 - j; s; s--) v /= 10;
        return '0' + v % 10;
    }
};

// ---- discovery: the paths of a batch's string values (k_json_paths, json_paths_emulate) ---------------------------------
constexpr uint32_t kJsonPathSlots = 1u << 16;      // the set of path hashes: open addressing, linear probing, 0: empty
constexpr uint32_t kJsonPathProbes = 128;          // ... given up behind this many slots (a full table: the path is dropped)
constexpr uint32_t kJsonPathCap = 16384;           // paths kept: more never compile into a trie (kJsonMaxNodes)
constexpr uint32_t kJsonPathPool = 8u << 20;       // bytes of the path pool
constexpr uint32_t kJsonPathMax = 65535;           // bytes of one path
constexpr uint64_t kJsonPathRoot = 0x243F6A8885A308D3ull;    // the hash of the path ""

// what a wave remembers of the containers it tracks, besides JsonWaveMem's kinds and count: allocated by discovery only
struct JsonPathMem {
    uint64_t pre_hash[kJsonMaxDepth];              // the hash of the container's own path ...
    uint32_t pre_len[kJsonMaxDepth];               // ... and its length in bytes, kJsonNone: it has none
    uint64_t cur_hash[kJsonMaxDepth];              // an object: the path of the member whose key was closed last
    uint32_t cur_len[kJsonMaxDepth];
    uint32_t key_off[kJsonMaxDepth];               // ... and where that key's bytes lie in the document
    uint32_t key_len[kJsonMaxDepth];
};
// the state of a batch: one allocation, cleared per call (the pool needs no clearing)
struct JsonPathSet {
    uint64_t* slots;                               // [kJsonPathSlots]
    uint32_t* count;                               // hashes that were new (may pass kJsonPathCap: the first kJsonPathCap own a number)
    uint32_t* dropped;                             // paths that were found and not written: cap, pool, probe limit
    uint32_t* cursor;                              // bytes of the pool handed out
    uint32_t* path_off;                            // [kJsonPathCap] where path n lies in the pool, kJsonNone: nowhere
    uint8_t* pool;                                 // per path: u32 length, the bytes, padded to 4
    uint32_t pool_bytes;
};

// A component's hash is a sum of per-byte terms, so that the lanes can add their shares in any order and host and device agree.
// The terms are 64 bits, mixed per (byte, position): json_key_term's sums collide by construction -- "1221" and "2112" give the
// same sum under its odd multipliers --, which the trie settles by comparing bytes and a set of hashes cannot.
GFT_JHD inline uint64_t json_path_term(uint32_t b, uint32_t j) {
    uint64_t x = (uint64_t)(b + 1u) * 0x9E3779B97F4A7C15ull + (uint64_t)(j + 1u) * 0xC2B2AE3D27D4EB4Full;
    x ^= x >> 32; x *= 0xD6E8FEB86659FD93ull; x ^= x >> 32;
    return x;
}
template <class W, class KB>
GFT_JHD inline uint64_t json_path_sum(W& w, const KB& kb, uint32_t len) {
    return w.sum64([&](uint32_t lane) {
        uint64_t s = 0;
        for (uint32_t j = lane; j < len; j += 64) s += json_path_term(kb(j), j);
        return s;
    });
}
// the path of a member under a container
GFT_JHD inline uint64_t json_path_mix(uint64_t parent, uint64_t h, uint32_t len) {
    uint64_t x = parent * 0x9E3779B97F4A7C15ull + h + (uint64_t)(len + 1u) * 0xC2B2AE3D27D4EB4Full;
    x ^= x >> 32; x *= 0xD6E8FEB86659FD93ull; x ^= x >> 29; x *= 0xD6E8FEB86659FD93ull; x ^= x >> 32;
    return x;
}
// (pre_hash, pre_len) + component -> (hash, len); len == kJsonNone: no path
template <class W, class KB>
GFT_JHD inline void json_path_child(W& w, uint64_t pre_hash, uint32_t pre_len, const KB& kb, uint32_t len, uint64_t& hash, uint32_t& plen) {
    plen = kJsonNone; hash = 0;
    if (pre_len == kJsonNone || len > kJsonPathMax) return;
    const uint32_t total = pre_len ? pre_len + 1 + len : len;          // (only the root's path is empty: components are not)
    if (total > kJsonPathMax) return;
    plen = total;
    hash = json_path_mix(pre_hash, json_path_sum(w, kb, len), len);
}

// child of `parent` under the component kb[0, len), or kJsonNone.  A hit is a node whose parent, length and bytes agree.
template <class W, class KB>
GFT_JHD inline uint32_t json_trie_find(W& w, const JsonTrie& T, uint32_t parent, const KB& kb, uint32_t len) {
    if (parent == kJsonNone || !len || len > T.max_key_len) return kJsonNone;
    const uint32_t h = w.sum([&](uint32_t lane) {
        uint32_t s = 0;
        for (uint32_t j = lane; j < len; j += 64) s += json_key_term(kb(j), j);
        return s;
    });
    for (uint32_t slot = json_slot_hash(parent, h) & T.table_mask;; slot = (slot + 1) & T.table_mask) {
        const uint32_t c = w.uni(T.table[slot]);
        if (c == kJsonNone) return kJsonNone;          // (the table is at most half full)
        JsonTrieNode nd = T.nodes[c];
        nd.parent = w.uni(nd.parent); nd.key_len = w.uni(nd.key_len); nd.key_off = w.uni(nd.key_off);
        if (nd.parent != parent || nd.key_len != len) continue;
        const uint64_t differ = w.ballot([&](uint32_t lane) {
            bool bad = false;
            for (uint32_t j = lane; j < len; j += 64) bad |= kb(j) != T.keys[nd.key_off + j];
            return bad;
        });
        if (!differ) return c;
    }
}

// ---- UTF-8, byte by byte (Go's utf8.DecodeRune: no overlong forms, no surrogates, nothing above U+10FFFF) -------------
// length of the valid sequence that d[i] leads, 0 if there is none inside the document
GFT_JHD inline uint32_t json_u8_seq(const uint8_t* d, uint32_t len, uint32_t i) {
    const uint32_t b0 = d[i];
    if (b0 < 0xC2 || b0 > 0xF4) return 0;
    const uint32_t need = b0 < 0xE0 ? 2u : b0 < 0xF0 ? 3u : 4u;
    if ((uint64_t)i + need > len) return 0;
    uint32_t lo = 0x80, hi = 0xBF;
    if (b0 == 0xE0) lo = 0xA0;
    if (b0 == 0xED) hi = 0x9F;
    if (b0 == 0xF0) lo = 0x90;
    if (b0 == 0xF4) hi = 0x8F;
    const uint32_t b1 = d[i + 1];
    if (b1 < lo || b1 > hi) return 0;
    if (need >= 3 && (d[i + 2] & 0xC0) != 0x80) return 0;
    if (need == 4 && (d[i + 3] & 0xC0) != 0x80) return 0;
    return need;
}
// is byte i (>= 0x80) part of a valid sequence?  A quote, a backslash and the document's ends are no continuation bytes, so a
// sequence never leaves the string it began in.
GFT_JHD inline bool json_u8_ok(const uint8_t* d, uint32_t len, uint32_t i) {
    if ((d[i] & 0xC0) != 0x80) return json_u8_seq(d, len, i) != 0;
    for (uint32_t k = 1; k <= 3 && k <= i; k++)
        if (json_u8_seq(d, len, i - k) > k) return true;
    return false;
}

GFT_JHD inline int json_hex(uint32_t c) {
    if (c - '0' < 10u) return (int)(c - '0');
    if ((c | 0x20) - 'a' < 6u) return (int)((c | 0x20) - 'a' + 10);
    return -1;
}

// ---- the masks of a piece --------------------------------------------------------------------------------------------
struct JsonMasks {
    uint64_t valid;        // bytes of the document
    uint64_t interior;     // bytes inside a string (between its quotes)
    uint64_t events;       // what the grammar sees: neither whitespace nor inside a string
    uint64_t syn;          // inside a string: a control byte, a bad escape, bad \u digits
    uint64_t bs;           // inside a string: backslashes
    uint64_t bad8;         // inside a string: a byte of no valid UTF-8 sequence
    uint64_t surr;         // inside a string: \uD800 .. \uDFFF
    uint64_t len0, len1;   // inside a string: bits 0 and 1 of the bytes a lane gives
};
struct JsonCarry { uint32_t escaped, in_string, hex; };      // from the piece in front

GFT_JHD inline uint64_t json_prefix_xor(uint64_t x) {
    x ^= x << 1; x ^= x << 2; x ^= x << 4; x ^= x << 8; x ^= x << 16; x ^= x << 32;
    return x;
}
GFT_JHD inline uint64_t json_range(uint32_t lo, uint32_t hi) {               // bits lo .. hi - 1, hi <= 64
    const uint64_t below_hi = hi >= 64 ? ~0ull : (1ull << hi) - 1;
    return lo >= 64 ? 0 : below_hi & ~((1ull << lo) - 1);
}
GFT_JHD inline uint32_t json_popc(uint64_t x) { return (uint32_t)__builtin_popcountll(x); }

template <class W>
GFT_JHD inline void json_piece_masks(W& w, const uint8_t* doc, uint32_t len, uint32_t base, JsonCarry& C, JsonMasks& M) {
    M.valid = len - base >= 64 ? ~0ull : (1ull << (len - base)) - 1;
    const uint64_t quote = w.ballot([&](uint32_t l) { return w.lane_byte(l) == '"'; }) & M.valid;
    uint64_t bs = w.ballot([&](uint32_t l) { return w.lane_byte(l) == '\\'; }) & M.valid;
    const uint64_t is_u = w.ballot([&](uint32_t l) { return w.lane_byte(l) == 'u'; }) & M.valid;
    // characters behind a backslash run of odd length (the run may have begun in the piece in front)
    const uint64_t all_bs = bs;
    bs &= ~(uint64_t)C.escaped;
    const uint64_t follows = bs << 1 | C.escaped;
    const uint64_t even = 0x5555555555555555ull;
    const uint64_t odd_starts = bs & ~even & ~follows;
    const uint64_t even_seq = odd_starts + bs;
    C.escaped = even_seq < odd_starts ? 1u : 0u;                                // (the run reaches the piece's end)
    const uint64_t escaped = (even ^ (even_seq << 1)) & follows;
    const uint64_t uq = quote & ~escaped;
    const uint64_t in_string = json_prefix_xor(uq) ^ (C.in_string ? ~0ull : 0ull);   // from an opening quote to the byte before the closing one
    C.in_string = (uint32_t)(in_string >> 63);
    M.interior = in_string & ~uq & M.valid;
    const uint64_t uesc = escaped & is_u & M.interior;
    const uint64_t hex = (uesc << 1 | uesc << 2 | uesc << 3 | uesc << 4 | C.hex) & M.interior;
    C.hex = (uint32_t)(uesc >> 63 | uesc >> 62 | uesc >> 61 | uesc >> 60);
    M.bs = all_bs & M.interior;
    enum : uint32_t { F_WS = 1, F_SYN = 2, F_BAD8 = 4, F_SURR = 8, F_L0 = 16, F_L1 = 32 };
    auto classify = [&](uint32_t l) -> uint32_t {
        JsonLaneOut& o = w.out(l);
        o.n = 0;
        const uint64_t bit = 1ull << l;
        if (!(M.valid & bit)) return 0;
        const uint32_t b = w.lane_byte(l);
        if (!(M.interior & bit)) return (b == ' ' || b == '\t' || b == '\n' || b == '\r') ? F_WS : 0;
        uint32_t f = b < 0x20 ? F_SYN : 0;
        if (escaped & bit) {
            o.n = 1;
            switch (b) {
            case '"': case '\\': case '/': o.o[0] = (uint8_t)b; break;
            case 'b': o.o[0] = 8; break;
            case 'f': o.o[0] = 12; break;
            case 'n': o.o[0] = 10; break;
            case 'r': o.o[0] = 13; break;
            case 't': o.o[0] = 9; break;
            case 'u': {
                o.n = 0;
                const uint64_t pos = (uint64_t)base + l;
                if (pos + 4 >= len) { f |= F_SYN; break; }                       // (no room for four digits and a closing quote)
                int cp = 0;
                for (uint32_t k = 1; k <= 4; k++) {
                    const int h = json_hex(doc[pos + k]);
                    if (h < 0) { f |= F_SYN; cp = 0; break; }
                    cp = cp * 16 + h;
                }
                if (f & F_SYN) break;
                if (cp >= 0xD800 && cp <= 0xDFFF) { f |= F_SURR; break; }
                if (cp < 0x80) { o.n = 1; o.o[0] = (uint8_t)cp; }
                else if (cp < 0x800) { o.n = 2; o.o[0] = (uint8_t)(0xC0 | cp >> 6); o.o[1] = (uint8_t)(0x80 | (cp & 63)); }
                else { o.n = 3; o.o[0] = (uint8_t)(0xE0 | cp >> 12); o.o[1] = (uint8_t)(0x80 | (cp >> 6 & 63)); o.o[2] = (uint8_t)(0x80 | (cp & 63)); }
                break;
            }
            default: o.n = 0; f |= F_SYN;
            }
        } else if (b != '\\' && !(hex & bit)) {
            o.n = 1; o.o[0] = (uint8_t)b;
            if (b >= 0x80 && !json_u8_ok(doc, len, base + l)) f |= F_BAD8;
        }
        return f | (o.n & 1 ? F_L0 : 0) | (o.n & 2 ? F_L1 : 0);
    };
    w.each([&](uint32_t l) { w.flags(l) = classify(l); });
    const uint64_t ws = w.ballot([&](uint32_t l) { return (w.flags(l) & F_WS) != 0; });
    M.syn = w.ballot([&](uint32_t l) { return (w.flags(l) & F_SYN) != 0; });
    M.bad8 = w.ballot([&](uint32_t l) { return (w.flags(l) & F_BAD8) != 0; });
    M.surr = w.ballot([&](uint32_t l) { return (w.flags(l) & F_SURR) != 0; });
    M.len0 = w.ballot([&](uint32_t l) { return (w.flags(l) & F_L0) != 0; });
    M.len1 = w.ballot([&](uint32_t l) { return (w.flags(l) & F_L1) != 0; });
    M.events = M.valid & ~M.interior & ~ws;
}

// ---- the grammar and the trie, wave-uniform ----------------------------------------------------------------------------
enum : uint32_t { kJwValue, kJwValueOrClose, kJwKeyOrClose, kJwKey, kJwColon, kJwAfter, kJwInString, kJwNumber, kJwLiteral };
enum : uint32_t { kJnMinus, kJnZero, kJnInt, kJnDot, kJnFrac, kJnE, kJnESign, kJnExp };
enum : uint32_t { kJmKey = 1, kJmLeaf = 2, kJmOther = 3 };

struct JsonWalk {
    uint32_t cond = 0;             // bit s: the condition of status s was met
    uint32_t state = kJwValue;
    uint32_t depth = 0;            // containers open
    uint32_t prev_pos = 0;         // offset of the event in front (numbers and literals end where the bytes stop being adjacent)
    uint32_t num = 0;              // state of the number, or characters of the literal read
    uint32_t lit = 0;              // the literal's first character
    uint32_t mode = 0;             // what the open string is
    uint32_t key_start = 0, key_bad = 0;
    uint32_t key_node = kJsonNone; // where the member's value sits
    uint32_t n_leaves = 0, n_text = 0;
};

// 0: c continues the number, 1: the number ended in front of c, 2: c cannot follow
GFT_JHD inline uint32_t json_num_step(uint32_t& s, uint32_t c) {
    const bool digit = c - '0' < 10u, e = (c | 0x20) == 'e';
    switch (s) {
    case kJnMinus: if (c == '0') { s = kJnZero; return 0; } if (digit) { s = kJnInt; return 0; } return 2;
    case kJnZero: if (c == '.') { s = kJnDot; return 0; } if (e) { s = kJnE; return 0; } return 1;
    case kJnInt: if (digit) return 0; if (c == '.') { s = kJnDot; return 0; } if (e) { s = kJnE; return 0; } return 1;
    case kJnDot: if (digit) { s = kJnFrac; return 0; } return 2;
    case kJnFrac: if (digit) return 0; if (e) { s = kJnE; return 0; } return 1;
    case kJnE: if (c == '+' || c == '-') { s = kJnESign; return 0; } if (digit) { s = kJnExp; return 0; } return 2;
    case kJnESign: if (digit) { s = kJnExp; return 0; } return 2;
    default: return digit ? 0 : 1;
    }
}
GFT_JHD inline bool json_num_done(uint32_t s) { return s == kJnZero || s == kJnInt || s == kJnFrac || s == kJnExp; }
GFT_JHD inline uint32_t json_lit_char(uint32_t lit, uint32_t k) {            // character k of true / false / null, 0 behind it
    const uint64_t word = lit == 't' ? 0x65757274ull : lit == 'f' ? 0x65736C6166ull : 0x6C6C756Eull;
    return k < 8 ? (uint32_t)(word >> (8 * k)) & 0xFF : 0;
}

template <class W>
GFT_JHD inline void json_mark(W& w, JsonWalk& S, uint32_t node) {
    if (node == kJsonNone) return;
    const uint32_t word = w.uni(w.mem().visited[node >> 5]);
    if (word >> (node & 31) & 1) S.cond |= 1u << kJsDup;
    w.mem().visited[node >> 5] = word | 1u << (node & 31);
}
template <class W>
GFT_JHD inline uint32_t json_parent(W& w, const JsonWalk& S) { return S.depth <= kJsonMaxDepth ? w.uni(w.mem().node[S.depth - 1]) : kJsonNone; }
template <class W>
GFT_JHD inline bool json_top_is_object(W& w, const JsonWalk& S) { return w.uni(w.mem().kinds[(S.depth - 1) >> 5]) >> ((S.depth - 1) & 31) & 1; }

// the node of the value that begins now: the root, the member's node, or the array element's
template <class W>
GFT_JHD inline uint32_t json_value_node(W& w, const JsonTrie& T, JsonWalk& S) {
    if (!S.depth) return 0;
    if (json_top_is_object(w, S)) return S.key_node;
    const uint32_t parent = json_parent(w, S);
    if (parent == kJsonNone) return kJsonNone;
    const JsonKeyIndex kb(w.uni(w.mem().count[S.depth - 1]));
    const uint32_t node = json_trie_find(w, T, parent, kb, kb.len());
    json_mark(w, S, node);
    return node;
}

// ---- discovery -------------------------------------------------------------------------------------------------------------
struct JsonNoPaths { static constexpr bool on = false; };
struct JsonPaths {                                 // what discovery reads and fills
    static constexpr bool on = true;
    JsonPathMem* pm;
    JsonPathSet set;
};

// the path of the value that begins now
template <class W, class D>
GFT_JHD inline void json_value_path(W& w, D& dsc, const JsonWalk& S, uint64_t& hash, uint32_t& plen) {
    if (!S.depth) { hash = kJsonPathRoot; plen = 0; return; }
    hash = 0; plen = kJsonNone;
    if (S.depth > kJsonMaxDepth) return;
    const uint32_t d = S.depth - 1;
    JsonPathMem& pm = *dsc.pm;
    if (json_top_is_object(w, S)) { hash = w.uni64(pm.cur_hash[d]); plen = w.uni(pm.cur_len[d]); return; }
    const JsonKeyIndex kb(w.uni(w.mem().count[d]));
    json_path_child(w, w.uni64(pm.pre_hash[d]), w.uni(pm.pre_len[d]), kb, kb.len(), hash, plen);
}

// A string value at the path (hash, plen), whose components the wave still holds.  The slot is read with a plain load first:
// a path that is in the set already -- the common case -- costs no atomic.  The wave whose compare-and-swap put the hash in
// takes a path number and pool space and writes the bytes with all its lanes; when the cap or the pool is exhausted the slot
// keeps the hash and nothing is written.  Nothing at or behind pool + pool_bytes is stored.
template <class W>
GFT_JHD inline void json_path_found(W& w, const JsonPathSet& G, JsonPathMem& pm, const uint8_t* doc, const JsonWalk& S, uint64_t hash, uint32_t plen) {
    if (!hash) hash = 1;
    uint32_t slot = (uint32_t)(hash >> 40) & (kJsonPathSlots - 1);
    for (uint32_t probe = 0; probe < kJsonPathProbes; probe++, slot = (slot + 1) & (kJsonPathSlots - 1)) {
        uint64_t v = w.load64(G.slots + slot);
        if (v == hash) return;
        if (v) continue;
        v = w.cas64(G.slots + slot, hash);                                     // (one lane; the slot's value before it)
        if (v == hash) return;
        if (v) continue;
        const uint32_t n = w.add32(G.count, 1);
        const uint32_t need = 4 + ((plen + 3) & ~3u);
        if (n >= kJsonPathCap) { (void)w.add32(G.dropped, 1); return; }
        const uint32_t off = w.add32(G.cursor, need);                          // (at most kJsonPathCap times: no wrap)
        if ((uint64_t)off + need > G.pool_bytes) { (void)w.add32(G.dropped, 1); return; }
        const uint32_t end = off + 4 + plen;
        uint32_t at = off + 4;
        for (uint32_t d = 0; d < S.depth; d++) {
            if (d) { w.once([&]() { if (at < end) G.pool[at] = '.'; }); at++; }
            auto put = [&](const auto& kb, uint32_t len) {
                w.each([&](uint32_t l) { for (uint32_t j = l; j < len; j += 64) if (at + j < end) G.pool[at + j] = (uint8_t)kb(j); });
                at += len;
            };
            if (w.uni(w.mem().kinds[d >> 5]) >> (d & 31) & 1) put(JsonKeyMem{doc + w.uni(pm.key_off[d])}, w.uni(pm.key_len[d]));
            else { const JsonKeyIndex kb(w.uni(w.mem().count[d])); put(kb, kb.len()); }
        }
        w.once([&]() { *reinterpret_cast<uint32_t*>(G.pool + off) = plen; G.path_off[n] = off; });   // (off is a multiple of 4)
        return;
    }
    (void)w.add32(G.dropped, 1);
}

// One event: byte c at offset pos of the document, outside every string or one of its quotes.  false: not JSON.
template <class W, class D>
GFT_JHD inline bool json_event(W& w, D& dsc, const JsonTrie& T, const uint8_t* doc, const JsonDocOut& O, JsonWalk& S, uint32_t pos, uint32_t c) {
    const uint32_t prev = S.prev_pos;
    S.prev_pos = pos;
    if (S.state == kJwNumber) {
        const uint32_t r = pos == prev + 1 ? json_num_step(S.num, c) : 1u;
        if (r == 0) return true;
        if (r == 2 || !json_num_done(S.num)) return false;
        S.state = kJwAfter;
    } else if (S.state == kJwLiteral) {
        if (pos != prev + 1 || c != json_lit_char(S.lit, S.num)) return false;
        if (!json_lit_char(S.lit, ++S.num)) S.state = kJwAfter;
        return true;
    }
    switch (S.state) {
    case kJwValue:
    case kJwValueOrClose:
        if (c == ']' && S.state == kJwValueOrClose) { S.depth--; S.state = kJwAfter; return true; }
        if (c == '"') {
            if constexpr (D::on) {
                uint64_t hash; uint32_t plen;
                json_value_path(w, dsc, S, hash, plen);
                if (plen != kJsonNone) json_path_found(w, dsc.set, *dsc.pm, doc, S, hash, plen);
                S.mode = kJmOther;
            } else {
                const uint32_t node = json_value_node(w, T, S);
                const uint32_t field = node == kJsonNone ? kJsonNone : w.uni(T.nodes[node].field);
                if (field == kJsonNone) { S.cond |= 1u << kJsPath; S.mode = kJmOther; }
                else {
                    S.mode = kJmLeaf;
                    const uint64_t l = O.leaf_base + S.n_leaves;
                    if (O.leaf_off && l < O.leaf_cap) w.once([&]() { O.leaf_field[l] = field; O.leaf_off[l] = O.text_base + S.n_text; });
                    S.n_leaves++;
                }
            }
            S.state = kJwInString;
            return true;
        }
        if (c == '{' || c == '[') {
            if (S.depth >= kJsonHardDepth) return false;                        // json_mini: "exceeded max depth"
            if constexpr (D::on) {
                if (S.depth < kJsonMaxDepth) {                                  // the container's own path, before it is pushed
                    uint64_t hash; uint32_t plen;
                    json_value_path(w, dsc, S, hash, plen);
                    dsc.pm->pre_hash[S.depth] = hash; dsc.pm->pre_len[S.depth] = plen; dsc.pm->cur_len[S.depth] = kJsonNone;
                }
            }
            uint32_t node = kJsonNone;
            if constexpr (!D::on) node = S.depth < kJsonMaxDepth ? json_value_node(w, T, S) : kJsonNone;
            const uint32_t kw = w.uni(w.mem().kinds[S.depth >> 5]);
            w.mem().kinds[S.depth >> 5] = c == '{' ? kw | 1u << (S.depth & 31) : kw & ~(1u << (S.depth & 31));
            if (S.depth < kJsonMaxDepth) { w.mem().node[S.depth] = node; w.mem().count[S.depth] = 0; }
            else S.cond |= 1u << kJsDepth;
            S.depth++;
            S.state = c == '{' ? kJwKeyOrClose : kJwValueOrClose;
            return true;
        }
        if (c == '-' || c - '0' < 10u) { S.state = kJwNumber; S.num = c == '-' ? kJnMinus : c == '0' ? kJnZero : kJnInt; return true; }
        if (c == 't' || c == 'f' || c == 'n') { S.state = kJwLiteral; S.lit = c; S.num = 1; return true; }
        return false;
    case kJwKeyOrClose:
        if (c == '}') { S.depth--; S.state = kJwAfter; return true; }
        [[fallthrough]];
    case kJwKey:
        if (c != '"') return false;
        S.mode = kJmKey; S.key_start = pos + 1; S.key_bad = 0; S.state = kJwInString;
        return true;
    case kJwColon:
        if (c != ':') return false;
        S.state = kJwValue;
        return true;
    case kJwAfter:
        if (!S.depth) return false;                                             // bytes after the top-level value
        if (json_top_is_object(w, S)) {
            if (c == ',') { S.state = kJwKey; return true; }
            if (c != '}') return false;
        } else {
            if (c == ',') { if (S.depth <= kJsonMaxDepth) w.mem().count[S.depth - 1] = w.uni(w.mem().count[S.depth - 1]) + 1; S.state = kJwValue; return true; }
            if (c != ']') return false;
        }
        S.depth--;
        return true;
    default:                                                                    // kJwInString: the closing quote
        if (S.mode == kJmKey) {
            const uint32_t len = pos - S.key_start;
            if (!len) { S.cond |= 1u << kJsKey; S.key_bad = 1; }
            if constexpr (D::on) {
                if (S.depth <= kJsonMaxDepth) {
                    const uint32_t d = S.depth - 1;
                    JsonPathMem& pm = *dsc.pm;
                    uint64_t hash = 0; uint32_t plen = kJsonNone;
                    if (!S.key_bad) json_path_child(w, w.uni64(pm.pre_hash[d]), w.uni(pm.pre_len[d]), JsonKeyMem{doc + S.key_start}, len, hash, plen);
                    pm.cur_hash[d] = hash; pm.cur_len[d] = plen; pm.key_off[d] = S.key_start; pm.key_len[d] = len;
                }
            } else {
                S.key_node = S.key_bad ? kJsonNone : json_trie_find(w, T, json_parent(w, S), JsonKeyMem{doc + S.key_start}, len);
                json_mark(w, S, S.key_node);
            }
            S.state = kJwColon;
        } else {
            S.state = kJwAfter;
        }
        S.mode = 0;
        return true;
    }
}

// the bytes m of the open string that lie in this piece
template <class W>
GFT_JHD inline void json_segment(W& w, const JsonMasks& M, const JsonDocOut& O, JsonWalk& S, uint64_t m) {
    if (S.mode == kJmKey) {
        if (m & (M.bs | M.bad8)) { S.cond |= 1u << kJsKey; S.key_bad = 1; }
    } else if (S.mode == kJmLeaf) {
        if (m & (M.bad8 | M.surr)) S.cond |= 1u << kJsText;
        const uint64_t l0 = M.len0 & m, l1 = M.len1 & m;
        if (O.text && (l0 | l1)) {
            const uint64_t at = O.text_base + S.n_text;
            w.each([&](uint32_t l) {
                const JsonLaneOut& o = w.out(l);
                if (!(m >> l & 1) || !o.n) return;
                const uint64_t below = (1ull << l) - 1;
                const uint64_t dst = at + json_popc(l0 & below) + 2 * json_popc(l1 & below);
                for (uint32_t q = 0; q < o.n; q++)
                    if (dst + q < O.text_cap) O.text[dst + q] = o.o[q];
            });
        }
        S.n_text += json_popc(l0) + 2 * json_popc(l1);
    }
}

// One document.  Returns its status; *n_leaves / *n_text: what it gives (0 unless the status is 0).
template <class W, class D = JsonNoPaths>
GFT_JHD inline uint32_t json_walk_doc(W& w, const JsonTrie& T, const uint8_t* doc, uint32_t len, const JsonDocOut& O, uint32_t* n_leaves,
                                      uint32_t* n_text, D dsc = D()) {
    *n_leaves = 0; *n_text = 0;
    if constexpr (!D::on) {
        const uint32_t words = (T.n_nodes + 31) / 32;
        w.each([&](uint32_t l) { for (uint32_t k = l; k < words; k += 64) w.mem().visited[k] = 0; });
    }
    JsonWalk S;
    JsonCarry C{0, 0, 0};
    JsonMasks M;
    for (uint64_t base = 0; base < len; base += 64) {
        w.load(doc, (uint32_t)base, len);
        json_piece_masks(w, doc, len, (uint32_t)base, C, M);
        if (M.syn) return kJsSyntax;
        uint32_t seg_lo = 0;
        for (uint64_t ev = M.events; ev; ev &= ev - 1) {
            const uint32_t k = (uint32_t)__builtin_ctzll(ev);
            if (S.state == kJwInString) json_segment(w, M, O, S, json_range(seg_lo, k));
            if (!json_event(w, dsc, T, doc, O, S, (uint32_t)base + k, w.byte_at(k))) return kJsSyntax;
            seg_lo = k + 1;
        }
        if (S.state == kJwInString) json_segment(w, M, O, S, json_range(seg_lo, 64) & M.valid);
    }
    if (S.state == kJwNumber && json_num_done(S.num)) S.state = kJwAfter;
    if (S.state != kJwAfter || S.depth) return kJsSyntax;                      // the empty document, an open string or container, ...
    if (S.cond) return (uint32_t)__builtin_ctz(S.cond);
    *n_leaves = S.n_leaves; *n_text = S.n_text;
    return kJsOk;
}
// discovery: the paths of the document's string values go into dsc.set
template <class W>
GFT_JHD inline void json_walk_paths(W& w, const JsonPaths& dsc, const uint8_t* doc, uint32_t len) {
    const JsonTrie no_trie{nullptr, nullptr, nullptr, 0, 0, 0};
    const JsonDocOut none{nullptr, nullptr, nullptr, 0, 0, 0, 0};
    uint32_t a, b;
    (void)json_walk_doc(w, no_trie, doc, len, none, &a, &b, dsc);
}

}  // namespace gft
