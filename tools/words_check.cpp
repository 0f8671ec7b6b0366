// words_check.cpp -- the word filter's logic (csrc/gft_words_piece.hpp, run on the host by filter_word_matches_host) against a
// naive predicate written here, under the address and undefined-behaviour sanitizers: a stand-alone program, CPU only.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I. tools/words_check.cpp \
//       gofindthem_amd/csrc/words_host.cpp -o build/words_check
//   build/words_check 300
//
// Every input and output lies in a heap block of exactly its size -- the offsets, the entries [0, off[n]) with poison in front of
// off[0], the four outputs of exactly the cap --, so a read outside them or a store at or past the cap is an error of the
// sanitizer.  The text block is lead + documents + slack, where lead and slack are LETTERS: a walk that looked at a byte outside
// its document would take a word rune for a neighbour and answer differently from the naive predicate, which is handed the
// document alone.  First the border cases: an occurrence at a document's first and last byte, a rune cut by the border on either
// side, keywords with an invalid byte at an edge, empty documents, lists of T - 1, T, T + 1 and 2T + 1 entries (T the entries of a
// tile).  Then N seeded random rounds over an alphabet of word runes, other runes and invalid sequences: both length sources,
// positions of first and of last bytes, a random lead and off[0], a random cap, one output dropped at random; then an entry put
// out of its document, a term id put out of range and an offset made to descend, which must be refused with every output
// untouched.  The naive predicate is Go's utf8.DecodeRune and utf8.DecodeLastRune written out statement by statement, with the
// classes of its own alphabet.  Exit code 0: walk and naive predicate agree everywhere.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "gofindthem_amd/csrc/gft_words.hpp"

using namespace gft;

namespace {

std::mt19937_64 rng;
uint64_t rnd(uint64_t n) { return n ? rng() % n : 0; }
int failures = 0;

template <class T>
std::unique_ptr<T[]> exact(const std::vector<T>& v) {
    std::unique_ptr<T[]> p(new T[v.size() ? v.size() : 1]);
    std::copy(v.begin(), v.end(), p.get());
    return p;
}

// ---- the naive side -----------------------------------------------------------------------------------------------------------
constexpr int32_t kRuneError = 0xFFFD;
struct Rune { int32_t r; int size; };

Rune decode_rune(const std::string& p) {
    const size_t n = p.size();
    if (n == 0) return {kRuneError, 0};
    const unsigned b0 = (unsigned char)p[0];
    if (b0 < 0x80) return {(int32_t)b0, 1};
    if (b0 < 0xC2 || b0 > 0xF4) return {kRuneError, 1};
    const int need = b0 < 0xE0 ? 2 : b0 < 0xF0 ? 3 : 4;
    unsigned lo = 0x80, hi = 0xBF;
    if (b0 == 0xE0) lo = 0xA0;
    if (b0 == 0xED) hi = 0x9F;
    if (b0 == 0xF0) lo = 0x90;
    if (b0 == 0xF4) hi = 0x8F;
    if ((int)n < need) return {kRuneError, 1};
    const unsigned b1 = (unsigned char)p[1];
    if (b1 < lo || b1 > hi) return {kRuneError, 1};
    int32_t cp = (int32_t)(b0 & (need == 2 ? 0x1F : need == 3 ? 0x0F : 0x07)) << 6 | (int32_t)(b1 & 0x3F);
    for (int k = 2; k < need; k++) {
        const unsigned b = (unsigned char)p[k];
        if ((b & 0xC0) != 0x80) return {kRuneError, 1};
        cp = cp << 6 | (int32_t)(b & 0x3F);
    }
    return {cp, need};
}

Rune decode_last_rune(const std::string& p) {
    const int end = (int)p.size();
    if (end == 0) return {kRuneError, 0};
    int start = end - 1;
    const unsigned r = (unsigned char)p[start];
    if (r < 0x80) return {(int32_t)r, 1};
    int lim = end - 4;
    if (lim < 0) lim = 0;
    for (start--; start >= lim; start--)
        if (((unsigned char)p[start] & 0xC0) != 0x80) break;
    if (start < 0) start = 0;
    const Rune d = decode_rune(p.substr(start, end - start));
    if (start + d.size != end) return {kRuneError, 1};
    return d;
}

// the alphabet: word runes, other runes, invalid sequences
const std::vector<std::string> kWordSyms = {"a", "b", "c", "_", "7", "Z", "\xC3\xA9", "\xC3\x9F", "\xD0\x96", "\xE4\xB8\xAD", "\xCC\x81", "\xC2\xBD",
                                            "\xF0\x9D\x92\x9C"};
const std::vector<int32_t> kWordRunes = {'a', 'b', 'c', '_', '7', 'Z', 0xE9, 0xDF, 0x416, 0x4E2D, 0x301, 0xBD, 0x1D49C, 0xEF};
const std::vector<std::string> kOtherSyms = {" ", "-", "+", ".", "'", "\n", "\xC2\xA0", "\xE2\x80\x94", "\xE2\x80\x9C", "\xE3\x80\x81",
                                             "\xF0\x9F\x98\x80", "\xEF\xBF\xBD", "\xFF", "\xA9", "\xC3", "\xC0\x80", "\xED\xA0\x80", "\xF4\x90\x80\x80"};

bool naive_word(const Rune& d) {
    if (d.size == 0 || d.r == kRuneError) return false;
    if (d.r < 0x80) return (d.r >= '0' && d.r <= '9') || (d.r >= 'a' && d.r <= 'z') || (d.r >= 'A' && d.r <= 'Z') || d.r == '_';
    return std::find(kWordRunes.begin(), kWordRunes.end(), d.r) != kWordRunes.end();
}

bool naive_kept(const std::string& D, size_t s, size_t e) {
    if (naive_word(decode_last_rune(D.substr(0, s))) && naive_word(decode_rune(D.substr(s, e - s)))) return false;
    if (naive_word(decode_last_rune(D.substr(s, e - s))) && naive_word(decode_rune(D.substr(e)))) return false;
    return true;
}

// ---- a list and a round ---------------------------------------------------------------------------------------------------------
struct Entry { uint32_t doc, start, len, term; };

struct Batch {
    std::vector<std::string> docs;
    std::vector<std::string> terms;
    std::vector<Entry> entries;       // grouped by document, ascending
};

void find_entries(Batch& B) {
    B.entries.clear();
    for (uint32_t d = 0; d < B.docs.size(); d++) {
        std::vector<Entry> here;
        for (uint32_t t = 0; t < B.terms.size(); t++) {
            if (B.terms[t].empty()) continue;
            for (size_t at = B.docs[d].find(B.terms[t]); at != std::string::npos; at = B.docs[d].find(B.terms[t], at + 1))
                here.push_back({d, (uint32_t)at, (uint32_t)B.terms[t].size(), t});
        }
        std::sort(here.begin(), here.end(), [](const Entry& a, const Entry& b) { return a.start != b.start ? a.start < b.start : a.term < b.term; });
        B.entries.insert(B.entries.end(), here.begin(), here.end());
    }
}

enum Break { kNone, kPastDoc, kBadTerm, kDescend };

// one call of the host walk over B against the naive predicate.  from_terms: the lengths come from the term table
void check(const char* what, const Batch& B, size_t lead, uint64_t e0, bool from_terms, bool pos_end, int64_t cap_arg, int drop, Break brk) {
    const uint64_t n_docs = B.docs.size(), n = B.entries.size();
    std::string text(lead, 'a');
    std::vector<uint64_t> doc_off(n_docs + 1, lead), off(n_docs + 1, 0);
    for (size_t d = 0; d < n_docs; d++) { text += B.docs[d]; doc_off[d + 1] = text.size(); }
    text += std::string(64, 'b');
    std::vector<uint32_t> pos(e0 + n, 0xDEADBEEFu), len(e0 + n, 0xDEADBEEFu), term(e0 + n, 0xDEADBEEFu), term_len(B.terms.size());
    for (size_t t = 0; t < B.terms.size(); t++) term_len[t] = (uint32_t)B.terms[t].size();
    std::vector<uint32_t> want_pos, want_len, want_term;
    std::vector<uint64_t> want_off(n_docs + 1, 0);
    for (uint64_t i = 0; i < n; i++) {
        const Entry& E = B.entries[i];
        off[E.doc + 1]++;
        pos[e0 + i] = pos_end ? E.start + E.len - 1u : E.start;
        len[e0 + i] = E.len; term[e0 + i] = E.term;
        if (naive_kept(B.docs[E.doc], E.start, E.start + E.len)) {
            want_off[E.doc + 1]++;
            want_pos.push_back(pos[e0 + i]); want_len.push_back(E.len); want_term.push_back(E.term);
        }
    }
    for (size_t d = 0; d < n_docs; d++) { off[d + 1] += off[d]; want_off[d + 1] += want_off[d]; }
    for (size_t d = 0; d <= n_docs; d++) off[d] += e0;
    if (brk == kPastDoc && n) {
        const uint64_t i = rnd(n);
        const Entry& E = B.entries[i];
        const uint32_t dl = (uint32_t)B.docs[E.doc].size();
        pos[e0 + i] = pos_end ? dl : dl + 1u - E.len;       // one byte behind the document's end
        if (!E.len) return;
    } else if (brk == kBadTerm && n) {
        term[e0 + rnd(n)] = (uint32_t)B.terms.size() + (uint32_t)rnd(3);
        if (!from_terms) return;
    } else if (brk == kDescend && n_docs >= 2 && off[1] > 0) {
        off[1 + rnd(n_docs - 1)] = off[0] > 0 && rnd(2) ? off[0] - 1 : 0;
        bool descends = off[n_docs] < off[0];
        for (size_t d = 0; d < n_docs; d++) descends |= off[d + 1] < off[d];
        if (!descends) return;
    } else if (brk != kNone) {
        return;
    }
    const uint64_t total_want = want_pos.size();
    const uint64_t cap = cap_arg < 0 ? total_want : (uint64_t)cap_arg;
    const auto b_text = exact(std::vector<uint8_t>(text.begin(), text.end()));
    const auto b_doc_off = exact(doc_off), b_off = exact(off);
    const auto b_pos = exact(pos), b_len = exact(len), b_term = exact(term), b_term_len = exact(term_len);
    const auto o_off = exact(std::vector<uint64_t>(n_docs + 1, 0x5A5A5A5A5A5A5A5Aull));
    const auto o_pos = exact(std::vector<uint32_t>(cap, 0x5A5A5A5Au)), o_len = exact(std::vector<uint32_t>(cap, 0x5A5A5A5Au)),
               o_term = exact(std::vector<uint32_t>(cap, 0x5A5A5A5Au));
    uint64_t total = 77;
    const int rc = filter_word_matches_host(b_text.get(), b_doc_off.get(), n_docs, b_off.get(), b_pos.get(), from_terms ? nullptr : b_len.get(),
                                            b_term.get(), from_terms ? b_term_len.get() : nullptr, from_terms ? (uint32_t)B.terms.size() : 0u,
                                            pos_end ? GFT_WORDS_POS_END : 0u, drop == 0 ? nullptr : o_off.get(), cap ? o_pos.get() : nullptr,
                                            drop == 1 || !cap ? nullptr : o_len.get(), drop == 2 || !cap ? nullptr : o_term.get(), cap, &total);
    auto fail = [&](const char* why) {
        failures++;
        std::fprintf(stderr, "FAIL %s: %s (docs %llu, entries %llu, lead %zu, e0 %llu, from_terms %d, pos_end %d, cap %llu, drop %d, break %d)\n", what, why,
                     (unsigned long long)n_docs, (unsigned long long)n, lead, (unsigned long long)e0, (int)from_terms, (int)pos_end,
                     (unsigned long long)cap, drop, (int)brk);
    };
    if (brk != kNone) {
        if (rc != GFT_E_INVALID || total != 0) return fail("a broken list was not refused");
        for (size_t d = 0; d <= n_docs; d++) if (o_off[d] != 0x5A5A5A5A5A5A5A5Aull) return fail("a refusal wrote the offsets");
        for (uint64_t k = 0; k < cap; k++)
            if (o_pos[k] != 0x5A5A5A5Au || o_len[k] != 0x5A5A5A5Au || o_term[k] != 0x5A5A5A5Au) return fail("a refusal wrote an entry");
        return;
    }
    if (rc != GFT_OK) return fail("refused");
    if (total != total_want) return fail("total");
    if (drop != 0)
        for (size_t d = 0; d <= n_docs; d++) if (o_off[d] != want_off[d]) return fail("offsets");
    for (uint64_t k = 0; k < cap; k++) {
        const bool in = k < total_want;
        if (o_pos[k] != (in ? want_pos[k] : 0x5A5A5A5Au)) return fail("positions");
        if (o_len[k] != (in && drop != 1 ? want_len[k] : 0x5A5A5A5Au)) return fail("lengths");
        if (o_term[k] != (in && drop != 2 ? want_term[k] : 0x5A5A5A5Au)) return fail("terms");
    }
}

void check_all_ways(const char* what, const Batch& B) {
    for (int from_terms = 0; from_terms < 2; from_terms++)
        for (int pos_end = 0; pos_end < 2; pos_end++) {
            check(what, B, 0, 0, from_terms, pos_end, -1, -1, kNone);
            check(what, B, 3, 5, from_terms, pos_end, -1, -1, kNone);
            check(what, B, 1, 0, from_terms, pos_end, 0, -1, kNone);
            check(what, B, 2, 1, from_terms, pos_end, 1, -1, kNone);
        }
}

std::string random_doc(uint32_t max_syms) {
    std::string d;
    for (uint32_t k = rnd(max_syms + 1); k; k--) d += rnd(2) ? kWordSyms[rnd(kWordSyms.size())] : kOtherSyms[rnd(kOtherSyms.size())];
    return d;
}

}  // namespace

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? std::atoi(argv[1]) : 100;
    rng.seed(20261020);
    const uint32_t T = kWordsTile;
    const std::string e = "\xC3\xA9", z = "\xE4\xB8\xAD";
    // the border cases
    {
        Batch B{{"ushers he she hers na\xC3\xAFve na \xE2\x80\x9Che\xE2\x80\x9D he\xE2\x80\x94she c++x c++ x"}, {"he", "she", "hers", "na", "c++"}, {}};
        find_entries(B);
        check_all_ways("sentence", B);
    }
    {
        Batch B{{"xab", "ab", "abx", "ab", "", "ab"}, {"ab"}, {}};
        find_entries(B);
        check_all_ways("edges", B);
    }
    {
        Batch B{{"ab" + e.substr(0, 1), e.substr(1) + "ab", "ab" + z.substr(0, 2), z.substr(2) + "ab", z.substr(0, 1) + "ab" + z.substr(0, 1), "a" + e, e + "a"},
                {"ab", "a" + e.substr(0, 1), e.substr(1) + "a", "a"}, {}};
        find_entries(B);
        check_all_ways("cut runes", B);
    }
    {
        Batch B{{"a\xFF" "a a", "\xFF" "a", "a\xFF", "_\xFF" "ab", "\xF4\x90\x80\x80" "a", "a\xED\xA0\x80"}, {"\xFF" "a", "a\xFF", "a", "\x80" "a", "a\xED"}, {}};
        find_entries(B);
        check_all_ways("invalid edges", B);
    }
    for (uint32_t n : {T - 1, T, T + 1, 2 * T + 1}) {
        std::string d;
        for (uint32_t i = 0; i < n; i++) d += i % 3 ? "ab " : "cab ";
        Batch B{{"", d, ""}, {"ab"}, {}};
        find_entries(B);
        check_all_ways("tiles", B);
        Batch C{{d.substr(0, d.size() / 2), "ab-ab_ab ab7", d}, {"ab"}, {}};
        find_entries(C);
        check_all_ways("straddle", C);
    }
    {
        Batch B{{"abc", ""}, {""}, {{0, 0, 0, 0}, {0, 1, 0, 0}, {0, 3, 0, 0}, {1, 0, 0, 0}}};
        check("zero length", B, 2, 0, true, false, -1, -1, kNone);
        check("zero length", B, 0, 3, false, false, -1, -1, kNone);
        Batch N{{}, {"ab"}, {}};
        check("no documents", N, 0, 0, true, false, -1, -1, kNone);
    }
    // seeded random rounds
    for (int r = 0; r < rounds; r++) {
        Batch B;
        const uint32_t n_docs = 1 + (uint32_t)rnd(r % 7 == 0 ? 400 : 40);
        for (uint32_t d = 0; d < n_docs; d++) B.docs.push_back(rnd(6) ? random_doc(r % 5 == 0 ? 120 : 30) : std::string());
        B.terms = {"ab", "a", "c+", "+b", e, "a" + e, "b c", "cab", "\xFF" "a", "Z", z};
        find_entries(B);
        const bool from_terms = rnd(2), pos_end = rnd(2);
        const size_t lead = rnd(20);
        const uint64_t e0 = rnd(3) ? 0 : rnd(9);
        check("random", B, lead, e0, from_terms, pos_end, -1, (int)rnd(4) - 1, kNone);
        check("random cap", B, lead, e0, from_terms, pos_end, (int64_t)rnd(B.entries.size() + 2), -1, kNone);
        check("random past", B, lead, e0, from_terms, pos_end, -1, -1, kPastDoc);
        check("random term", B, lead, e0, true, pos_end, -1, -1, kBadTerm);
        check("random descend", B, lead, e0, from_terms, pos_end, -1, -1, kDescend);
    }
    if (failures) {
        std::fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    std::printf("words_check: border cases and %d random rounds agree with the naive predicate\n", rounds);
    return 0;
}
