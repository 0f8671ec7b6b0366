// lowermap_check.cpp -- the span map's logic (csrc/gft_lowermap_piece.hpp and tolower_piece_rune_at of csrc/gft_tolower_piece.hpp, run
// on the host by lowermap_host) against a sequential decoder written here, under the address and undefined-behaviour sanitizers:
// a stand-alone program, CPU only.  The sources include the HIP headers, so the compiler is hipcc, host side only:
//
//   hipcc -x hip --offload-host-only -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I. \
//       tools/lowermap_check.cpp gofindthem_amd/csrc/lowermap_host.cpp gofindthem_amd/csrc/tolower_host.cpp \
//       gofindthem_amd/csrc/dsl_compile.cpp -o build/lowermap_check
//   build/lowermap_check 300
//
// Every input and output lies in a heap block of exactly its size -- the text of doc_off[n] + 64 bytes (the slack the walk asks
// for), the offsets, the span arrays --, so a read outside them or a store past an array is an error of the sanitizer.  Fixed edge
// inputs first: the empty batch member, documents of one byte, every length-changing rune and every kind of invalid byte with its
// first byte at each offset around the piece (16), trip (1024) and unit (8192) borders and around the cut between the two units of
// a longer document, a non-zero doc_off[0] behind lead bytes that would complete a rune.  Then N seeded random rounds.  Each
// batch: EVERY single-byte span of every lowered document, the whole-document span, empty spans (at the lowered end too) and
// random ones, mapped by the walk and by the decoder; the same with a limit that leaves the tail of the arrays alone; and one span
// made a byte too long, which must be refused with both arrays untouched.  Every batch draws a span base s0, 0 among the values:
// span_off[0] = s0, the span arrays are blocks of exactly s0 + n entries whose first s0 hold a span no document could hold and
// must come back as they were, the decoder's answer is indexed the same way, and the limit is an index into these arrays.
// Exit code 0: walk and decoder agree everywhere.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "gofindthem_amd/csrc/gft_lowermap.hpp"

using namespace gft;

namespace {

std::mt19937_64 rng;
uint64_t rnd(uint64_t n) { return n ? rng() % n : 0; }

template <class T>
std::unique_ptr<T[]> exact(const std::vector<T>& v) {
    std::unique_ptr<T[]> p(new T[v.size() ? v.size() : 1]);
    for (size_t i = 0; i < v.size(); i++) p[i] = v[i];
    return p;
}

int fails = 0;
uint64_t runs = 0, spans_seen = 0;

// ---- Go's utf8.DecodeRune, byte after byte ------------------------------------------------------------------------------------
struct Rune { uint32_t a, sl, b, ll; };

bool cont(const std::string& s, size_t i, uint8_t lo = 0x80, uint8_t hi = 0xBF) { return i < s.size() && (uint8_t)s[i] >= lo && (uint8_t)s[i] <= hi; }

uint32_t utf8_len(uint32_t cp) { return cp < 0x80 ? 1 : cp < 0x800 ? 2 : cp < 0x10000 ? 3 : 4; }

std::vector<Rune> decode(const std::string& s, uint32_t* B) {
    const LowerTable T = lower_table_host().view();
    std::vector<Rune> out;
    uint32_t b = 0;
    for (size_t i = 0; i < s.size();) {
        const uint8_t c = (uint8_t)s[i];
        uint32_t n = 1, cp = c;
        bool ok = c < 0x80;
        if (c >= 0xC2 && c <= 0xDF && cont(s, i + 1)) {
            ok = true; n = 2; cp = (c & 0x1Fu) << 6 | ((uint8_t)s[i + 1] & 0x3Fu);
        } else if (c >= 0xE0 && c <= 0xEF && cont(s, i + 1, c == 0xE0 ? 0xA0 : 0x80, c == 0xED ? 0x9F : 0xBF) && cont(s, i + 2)) {
            ok = true; n = 3; cp = (c & 0x0Fu) << 12 | ((uint8_t)s[i + 1] & 0x3Fu) << 6 | ((uint8_t)s[i + 2] & 0x3Fu);
        } else if (c >= 0xF0 && c <= 0xF4 && cont(s, i + 1, c == 0xF0 ? 0x90 : 0x80, c == 0xF4 ? 0x8F : 0xBF) && cont(s, i + 2) && cont(s, i + 3)) {
            ok = true; n = 4; cp = (c & 0x07u) << 18 | ((uint8_t)s[i + 1] & 0x3Fu) << 12 | ((uint8_t)s[i + 2] & 0x3Fu) << 6 | ((uint8_t)s[i + 3] & 0x3Fu);
        }
        const uint32_t ll = ok ? utf8_len(tolower_rune(T, cp)) : 3;
        out.push_back(Rune{(uint32_t)i, n, b, ll});
        b += ll;
        i += n;
    }
    *B = b;
    return out;
}

struct Batch {
    std::vector<std::string> docs;
    uint64_t lead = 0;
};

void check_batch(const Batch& bt, const char* what) {
    const uint64_t n_docs = bt.docs.size();
    std::vector<uint64_t> off(n_docs + 1, bt.lead);
    std::vector<uint8_t> text(bt.lead, 0xC3);
    for (uint64_t d = 0; d < n_docs; d++) {
        text.insert(text.end(), bt.docs[d].begin(), bt.docs[d].end());
        off[d + 1] = text.size();
    }
    text.insert(text.end(), 64, 0x89);                              // slack that would complete a rune
    static const uint64_t base[] = {0, 0, 1, 2, kMapTile - 1, kMapTile, kMapTile + 1, 3 * kMapTile + 5};
    const uint64_t s0 = rnd(9) < 8 ? base[rnd(8)] : rnd(600);
    std::vector<uint64_t> so(n_docs + 1, s0);
    std::vector<uint32_t> st(s0, 0xFFFFFFFFu), ln(st), want_st(st), want_ln(st);
    for (uint64_t d = 0; d < n_docs; d++) {
        uint32_t B = 0;
        const std::vector<Rune> rs = decode(bt.docs[d], &B);
        std::vector<uint32_t> rune_of(B);
        for (size_t r = 0; r < rs.size(); r++)
            for (uint32_t k = 0; k < rs[r].ll; k++) rune_of[rs[r].b + k] = (uint32_t)r;
        auto add = [&](uint32_t s, uint32_t n) {
            st.push_back(s); ln.push_back(n);
            if (s == B) { want_st.push_back((uint32_t)bt.docs[d].size()); want_ln.push_back(0); return; }
            const Rune& p = rs[rune_of[s]];
            want_st.push_back(p.a);
            if (!n) { want_ln.push_back(0); return; }
            const Rune& q = rs[rune_of[s + n - 1]];
            want_ln.push_back(q.a + q.sl - p.a);
        };
        const bool all = B <= 3000;                                // every byte of the shorter documents, a sample of the longer
        for (uint32_t s = 0; s < B; s += all ? 1 : 1 + (uint32_t)rnd(40)) add(s, 1);
        add(0, B);
        add(B, 0);
        for (int k = 0; k < 40; k++) {
            const uint32_t s = (uint32_t)rnd((uint64_t)B + 1);
            add(s, (uint32_t)rnd(std::min<uint64_t>(B - s, 50) + 1));
        }
        so[d + 1] = st.size();
    }
    const uint64_t n = st.size() - s0, end = st.size();
    spans_seen += n;
    auto p_text = exact(text);
    auto p_off = exact(off);
    auto p_so = exact(so);
    auto run = [&](const std::vector<uint32_t>& a, const std::vector<uint32_t>& b, uint64_t limit, std::vector<uint32_t>& ga, std::vector<uint32_t>& gb) {
        auto pa = exact(a), pb = exact(b);
        const int rc = lowermap_host(p_text.get(), p_off.get(), n_docs, p_so.get(), pa.get(), pb.get(), limit);
        ga.assign(pa.get(), pa.get() + a.size());
        gb.assign(pb.get(), pb.get() + b.size());
        runs++;
        return rc;
    };
    std::vector<uint32_t> ga, gb;
    if (run(st, ln, ~0ull, ga, gb) != GFT_OK || ga != want_st || gb != want_ln) {
        for (uint64_t k = 0; k < end && k < ga.size(); k++)
            if (ga[k] != want_st[k] || gb[k] != want_ln[k]) {
                fprintf(stderr, "%s: span %llu (%u, %u): walk (%u, %u), decoder (%u, %u)\n", what, (unsigned long long)k, st[k], ln[k], ga[k], gb[k],
                        want_st[k], want_ln[k]);
                break;
            }
        fails++;
        return;
    }
    if (!n) return;
    // a limit: the entries at and past it are left alone
    const uint64_t limit = rnd(end + 2);                            // (below s0, inside, at the end and past it)
    if (run(st, ln, limit, ga, gb) != GFT_OK) { fprintf(stderr, "%s: refused under a limit\n", what); fails++; return; }
    for (uint64_t k = 0; k < end; k++) {
        const bool ok = k < limit ? ga[k] == want_st[k] && gb[k] == want_ln[k] : ga[k] == st[k] && gb[k] == ln[k];
        if (!ok) { fprintf(stderr, "%s: limit %llu, entry %llu\n", what, (unsigned long long)limit, (unsigned long long)k); fails++; return; }
    }
    // one span a byte too long: refused, nothing written
    {
        std::vector<uint32_t> bad_ln = ln;
        const uint64_t d = rnd(n_docs);
        const uint64_t k = so[d] + rnd(so[d + 1] - so[d]);
        uint32_t B = 0;
        decode(bt.docs[d], &B);
        bad_ln[k] = B - st[k] + 1;
        if (run(st, bad_ln, ~0ull, ga, gb) != GFT_E_INVALID || ga != st || gb != bad_ln) {
            fprintf(stderr, "%s: a span past the lowered end was taken, or the refusal wrote\n", what);
            fails++;
        }
    }
    if (s0) {                                                       // span_off[n_docs] < span_off[0]
        std::vector<uint64_t> down(so);
        down.back() = s0 - 1;
        auto p_down = exact(down);
        auto pa = exact(st), pb = exact(ln);
        const int rc = lowermap_host(p_text.get(), p_off.get(), n_docs, p_down.get(), pa.get(), pb.get(), ~0ull);
        if (rc != GFT_E_INVALID || memcmp(pa.get(), st.data(), end * 4) || memcmp(pb.get(), ln.data(), end * 4)) {
            fprintf(stderr, "%s: span offsets that descend were taken, or the refusal wrote\n", what);
            fails++;
        }
    }
}

std::string ascii(size_t n, uint64_t seed) {
    std::mt19937_64 g(seed);
    static const char alphabet[] = "ABCDEFXYZ abcdexyz,.09@[`{";
    std::string s(n, ' ');
    for (auto& c : s) c = alphabet[g() % (sizeof(alphabet) - 1)];
    return s;
}

const std::vector<std::string>& special_runes() {
    static const std::vector<std::string> v = {
        "\xC4\xB0", "\xE2\x84\xAA", "\xE1\xBA\x9E", "\xE2\x84\xA6", "\xC8\xBA", "\xC8\xBE", "\xC3\x89", "\xF0\x90\x90\x80", "\xEF\xBF\xBD",
        "\xC0\x80", "\xE0\x80\x80", "\xED\xA0\x80", "\xF4\x90\x80\x80", "\xC1\xBF", "\xF0\x80\x80\x80", "\x80", "\xBF", "\xE2\x82", "\xF0\x9F\x98", "\xC3",
        "\xF5", "\xFF"};
    return v;
}

void edges() {
    Batch tiny;
    tiny.docs = {"", "K", "\xFF", "\xC4\xB0", "", "\xA9 behind the lead", "ends with a lead \xC3"};
    for (uint64_t lead : {0, 1, 3, 17}) {
        tiny.lead = lead;
        check_batch(tiny, "tiny documents");
    }
    Batch none;
    check_batch(none, "no documents");
    const uint64_t unit_doc = kLowerUnitMax + 108, cut = (unit_doc + 1) / 2;
    for (uint64_t k : {(uint64_t)kLowerPiece, (uint64_t)kLowerChunk, (uint64_t)kLowerUnitMax, cut}) {
        Batch b;
        b.lead = k & 7;
        for (const std::string& r : special_runes())
            for (size_t j = 0; j < r.size(); j++) {
                std::string d = ascii(k - j, k + j) + r + ascii(40, j);
                if (k == cut) d += ascii(unit_doc - d.size(), 3);
                b.docs.push_back(d);
            }
        check_batch(b, "runes at a border");
    }
}

void one_round(int round) {
    Batch b;
    b.lead = rnd(4) ? rnd(40) : 0;
    const uint64_t n_docs = 1 + rnd(12);
    for (uint64_t d = 0; d < n_docs; d++) {
        const uint64_t want = rnd(8) ? rnd(300) : rnd(3) ? rnd(3000) : kLowerUnitMax - 20 + rnd(9000);
        std::string s;
        while (s.size() < want) {
            const uint64_t x = rnd(100);
            if (x < 55) s += ascii(1 + rnd(20), rng());
            else if (x < 85) s += special_runes()[rnd(special_runes().size())];
            else s += (char)(0x80 + rnd(0x80));
        }
        s.resize(want);
        b.docs.push_back(s);
    }
    char what[32];
    snprintf(what, sizeof what, "round %d", round);
    check_batch(b, what);
}

}  // namespace

int main(int argc, char** argv) {
    const int n = argc > 1 ? atoi(argv[1]) : 100;
    rng.seed(7);
    edges();
    for (int round = 0; round < n && !fails; round++) {
        rng.seed(20261020u + (uint64_t)round);
        one_round(round);
    }
    if (fails) { fprintf(stderr, "lowermap_check: %d failure(s)\n", fails); return 1; }
    printf("lowermap_check: walk and decoder agree (%llu runs of the walk, %llu spans)\n", (unsigned long long)runs, (unsigned long long)spans_seen);
    return 0;
}
