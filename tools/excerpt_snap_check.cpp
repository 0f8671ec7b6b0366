// excerpt_snap_check.cpp -- the snapped excerpts' logic (the word and line walks of csrc/gft_excerpt_piece.hpp, run on the host by
// excerpt_spans_snap_host) against a naive edge function and an independent union of intervals written here, under the address
// and undefined-behaviour sanitizers: a stand-alone program, CPU only.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I. tools/excerpt_snap_check.cpp \
//       gofindthem_amd/csrc/excerpt_host.cpp gofindthem_amd/csrc/words_host.cpp -o build/excerpt_snap_check
//   build/excerpt_snap_check 300
//
// Every input and output lies in a heap block of exactly its size, so a read outside them or a store past a cap is an error of
// the sanitizer.  The text is one block: lead bytes, the documents, and bytes behind the last document -- the lead and the tail
// hold word bytes ('a', or the first / last bytes of a two-byte letter), so a walk that left its document would go on there and
// disagree with the naive function, which is handed a COPY of the document alone.  The naive edge function decodes forwards from
// the document's first byte, Go's way: every byte starts a valid sequence of a word rune, of another rune, or is an error of one
// byte; a position cuts a word when a word rune ends there and one begins there.  It then walks as the contract says.  N seeded
// rounds: random documents over ASCII letters, digits, spaces, newlines, two-, three- and four-byte letters, symbols and invalid
// bytes; random before / after, flags (the three bits in their valid combinations) and reach (0, small, GFT_EXCERPT_REACH_MAX,
// with words and lines longer than it now and then); a span base; exact caps, count only and caps that cut.  Then the refusals.
// Exit code 0: walk and brute force agree everywhere.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "gofindthem_amd/csrc/gft_excerpt.hpp"
#include "gofindthem_amd/csrc/gft_words.hpp"

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
void expect(bool ok, const char* what, uint64_t round) {
    if (ok) return;
    std::fprintf(stderr, "round %llu: %s\n", (unsigned long long)round, what);
    fails++;
}

// ---- the naive edge function ---------------------------------------------------------------------------------------------------
// per position of the document: does a word rune begin here (and how long is it), does one end here (and how long was it)
struct Runes {
    std::vector<uint32_t> begins, ends;    // the size of the word rune, 0: none
};

// Go's DecodeRune on d[p ..): the size of a valid sequence and its code point, or 0
uint32_t decode(const std::vector<uint8_t>& d, size_t p, uint32_t& cp) {
    const size_t n = d.size() - p;
    const uint32_t b0 = d[p];
    if (b0 < 0x80) { cp = b0; return 1; }
    if (b0 < 0xC2 || b0 > 0xF4) return 0;
    const uint32_t need = b0 < 0xE0 ? 2 : b0 < 0xF0 ? 3 : 4;
    if (n < need) return 0;
    uint32_t lo = 0x80, hi = 0xBF;
    if (b0 == 0xE0) lo = 0xA0;
    if (b0 == 0xED) hi = 0x9F;
    if (b0 == 0xF0) lo = 0x90;
    if (b0 == 0xF4) hi = 0x8F;
    if (d[p + 1] < lo || d[p + 1] > hi) return 0;
    cp = b0 & (need == 2 ? 0x1F : need == 3 ? 0x0F : 0x07);
    for (uint32_t k = 1; k < need; k++) {
        if ((d[p + k] & 0xC0) != 0x80) return 0;
        cp = cp << 6 | (d[p + k] & 0x3F);
    }
    return need;
}

// a word rune begins at p: judged at p alone.  A word rune ends at p: DecodeLastRune's own search, written out -- the first rune
// start among the three bytes in front of the last one, the sequence there must end at p
Runes runes_of(const std::vector<uint8_t>& d) {
    Runes R;
    const size_t L = d.size();
    R.begins.assign(L + 1, 0);
    R.ends.assign(L + 1, 0);
    for (size_t p = 0; p < L; p++) {
        uint32_t cp = 0;
        const uint32_t n = decode(d, p, cp);
        if (n && words_is_word(word_table_host(), cp)) R.begins[p] = n;
    }
    for (size_t p = 1; p <= L; p++) {
        if (d[p - 1] < 0x80) { R.ends[p] = R.begins[p - 1] == 1 ? 1 : 0; continue; }
        if (d[p - 1] >= 0xC0) continue;
        for (size_t k = 1; k <= 3 && k < p; k++) {
            if ((d[p - 1 - k] & 0xC0) == 0x80) continue;
            // the slice is d[0 .. p): the sequence must fit in it and end at p
            std::vector<uint8_t> slice(d.begin(), d.begin() + p);
            uint32_t cp = 0;
            const uint32_t n = decode(slice, p - 1 - k, cp);
            if (n == k + 1 && words_is_word(word_table_host(), cp)) R.ends[p] = n;
            break;
        }
    }
    return R;
}

bool cont(uint8_t b) { return (b & 0xC0) == 0x80; }

void naive_edges(const std::vector<uint8_t>& d, const Runes& R, uint32_t flags, uint32_t reach, uint64_t& lo, uint64_t& hi) {
    const uint64_t L = d.size();
    if (flags & (GFT_EXCERPT_RUNES | GFT_EXCERPT_WORDS)) {
        for (int k = 0; k < 3 && lo > 0 && lo < L && cont(d[lo]); k++) lo--;
        for (int k = 0; k < 3 && hi < L && cont(d[hi]); k++) hi++;
    }
    if (flags & GFT_EXCERPT_WORDS) {
        auto cuts = [&](uint64_t p) { return p > 0 && p < L && R.ends[p] && R.begins[p]; };
        uint64_t p = lo;
        while (cuts(p)) {
            const uint64_t r = R.ends[p];
            if (lo - (p - r) > reach) { p = lo; break; }
            p -= r;
        }
        const uint64_t start = p;
        p = hi;
        while (cuts(p)) {
            const uint64_t r = R.begins[p];
            if ((p + r) - hi > reach) { p = hi; break; }
            p += r;
        }
        lo = start;
        hi = p;
    } else if (flags & GFT_EXCERPT_LINES) {
        uint64_t p = lo;
        while (p > 0 && d[p - 1] != '\n') {
            if (lo - (p - 1) > reach) { p = lo; break; }
            p--;
        }
        const uint64_t start = p;
        p = hi;
        while (p < L && d[p] != '\n') {
            if ((p + 1) - hi > reach) { p = hi; break; }
            p++;
        }
        lo = start;
        hi = p;
    }
}

// ---- batches --------------------------------------------------------------------------------------------------------------------
struct Batch {
    std::vector<uint8_t> text;             // lead, documents, tail
    std::vector<uint64_t> doc_off, span_off;
    std::vector<uint32_t> start, len;
    uint32_t before, after, flags, reach;
    uint64_t s0 = 0;
};

struct Result {
    std::vector<uint8_t> out;
    std::vector<uint64_t> exc_off, exc_doc, exc_span_off, doc_exc_off;
    std::vector<uint32_t> exc_start, span_rel;
};

constexpr uint32_t kPoison = 0xFFFFFFFFu, kUntouched = 0xA5A5A5A5u;

void put(std::vector<uint8_t>& t, const char* s) { while (*s) t.push_back((uint8_t)*s++); }

void random_symbol(std::vector<uint8_t>& t) {
    static const char* sym[] = {"a", "b", "Z", "7", "_", " ", " ", "-", ".", "\n", "\r", "\xc3\xa9", "\xd0\x96", "\xe4\xb8\xad", "\xcc\x81",
                                "\xf0\x9d\x92\x9c", "\xe2\x80\x94", "\xf0\x9f\x98\x80", "\xef\xbf\xbd", "\xff", "\xa9", "\xc3", "\xc0\x80",
                                "\xed\xa0\x80", "\xf4\x90\x80\x80", "\xe4\xb8"};
    put(t, sym[rnd(sizeof sym / sizeof *sym)]);
}

Batch random_batch(uint64_t n_docs, uint64_t max_symbols, uint64_t max_spans, bool long_runs) {
    Batch B;
    static const uint32_t away[] = {0, 0, 1, 2, 3, 5, 9, 40, 0xFFFFFFFFu};
    static const uint32_t reaches[] = {0, 1, 2, 3, 5, 64, 100, GFT_EXCERPT_REACH_MAX};
    static const uint32_t flagset[] = {0, 1, 2, 3, 4, 5, 2, 4};
    B.before = away[rnd(9)];
    B.after = away[rnd(9)];
    B.flags = flagset[rnd(8)];
    B.reach = long_runs ? GFT_EXCERPT_REACH_MAX : reaches[rnd(8)];
    static const uint64_t base[] = {0, 0, 1, 2, kExcTile - 1, kExcTile, kExcTile + 1};
    B.s0 = base[rnd(7)];
    B.start.assign(B.s0, kPoison);
    B.len.assign(B.s0, kPoison);
    // the lead: word bytes, the last of them the first byte of a two-byte letter now and then
    for (uint64_t k = rnd(6); k > 0; k--) B.text.push_back('a');
    if (rnd(3) == 0) B.text.push_back(0xC3);
    B.doc_off.push_back(B.text.size());
    B.span_off.push_back(B.s0);
    for (uint64_t d = 0; d < n_docs; d++) {
        const size_t a = B.text.size();
        if (rnd(5)) {
            if (long_runs && rnd(2)) {                             // a word or a line round the reach
                const uint64_t n = GFT_EXCERPT_REACH_MAX - 3 + rnd(8);
                for (uint64_t i = 0; i < n; i++) B.text.push_back(rnd(50) ? 'a' : (B.flags & GFT_EXCERPT_LINES ? ' ' : 'b'));
            }
            for (uint64_t k = rnd(max_symbols + 1); k > 0; k--) random_symbol(B.text);
        }
        const uint64_t L = B.text.size() - a;
        B.doc_off.push_back(B.text.size());
        std::vector<uint64_t> ends;
        for (uint64_t k = rnd(4) ? rnd(max_spans + 1) : 0; k > 0; k--) ends.push_back(rnd(L + 1));
        std::sort(ends.begin(), ends.end());
        for (uint64_t e : ends) {
            const uint64_t n = rnd(std::min<uint64_t>(e, 12) + 1);
            B.start.push_back((uint32_t)(e - n));
            B.len.push_back((uint32_t)n);
        }
        B.span_off.push_back(B.start.size());
    }
    // behind the last document: the second byte of a two-byte letter now and then, word bytes
    if (rnd(3) == 0) B.text.push_back(0xA9);
    for (uint64_t k = rnd(6); k > 0; k--) B.text.push_back('a');
    return B;
}

// the contract, by brute force: naive windows, a grid of whole and half positions per document
Result brute(const Batch& B) {
    Result R;
    const uint64_t n_docs = B.doc_off.size() - 1;
    R.exc_off.push_back(0);
    R.doc_exc_off.push_back(0);
    R.span_rel.assign(B.start.size(), kUntouched);
    for (uint64_t d = 0; d < n_docs; d++) {
        const std::vector<uint8_t> doc(B.text.begin() + B.doc_off[d], B.text.begin() + B.doc_off[d + 1]);   // a copy: nothing round it
        const uint64_t L = doc.size();
        const Runes runes = (B.flags & GFT_EXCERPT_WORDS) ? runes_of(doc) : Runes();
        std::vector<uint8_t> grid(2 * L + 1, 0);
        std::vector<std::pair<uint64_t, uint64_t>> win;
        for (uint64_t s = B.span_off[d]; s < B.span_off[d + 1]; s++) {
            uint64_t lo = B.start[s] > B.before ? (uint64_t)B.start[s] - B.before : 0;
            uint64_t hi = (uint64_t)B.start[s] + B.len[s] + B.after;
            if (hi > L) hi = L;
            naive_edges(doc, runes, B.flags, B.reach, lo, hi);
            win.emplace_back(lo, hi);
            for (uint64_t p = 2 * lo; p <= 2 * hi; p++) grid[p] = 1;
        }
        std::vector<std::pair<uint64_t, uint64_t>> runs;
        for (uint64_t p = 0; p <= 2 * L; p++) {
            if (!grid[p]) continue;
            uint64_t q = p;
            while (q + 1 <= 2 * L && grid[q + 1]) q++;
            runs.emplace_back(p / 2, q / 2);
            p = q;
        }
        std::vector<uint64_t> first_span(runs.size(), ~0ull);
        for (uint64_t s = B.span_off[d]; s < B.span_off[d + 1]; s++) {
            const auto& w = win[s - B.span_off[d]];
            const uint64_t r = std::upper_bound(runs.begin(), runs.end(), std::pair<uint64_t, uint64_t>(w.first, ~(uint64_t)0)) - runs.begin() - 1;
            if (!(runs[r].first <= w.first && w.second <= runs[r].second)) std::abort();
            if (first_span[r] == ~0ull) first_span[r] = s;
            R.span_rel[s] = (uint32_t)(B.start[s] - runs[r].first);
        }
        for (size_t r = 0; r < runs.size(); r++) {
            R.exc_doc.push_back(d);
            R.exc_start.push_back((uint32_t)runs[r].first);
            R.exc_span_off.push_back(first_span[r]);
            R.out.insert(R.out.end(), doc.begin() + runs[r].first, doc.begin() + runs[r].second);
            R.exc_off.push_back(R.out.size());
        }
        R.doc_exc_off.push_back(R.exc_doc.size());
    }
    R.exc_span_off.push_back(B.span_off[n_docs]);
    return R;
}

// the walk under (cap_bytes, cap_exc) into blocks of exactly those sizes; compared with the brute force up to the caps
void check(const Batch& B, const Result& want, uint64_t cap_bytes, uint64_t cap_exc, uint64_t round) {
    const uint64_t n_docs = B.doc_off.size() - 1, m = want.exc_doc.size(), total = want.out.size();
    auto text = exact(B.text);
    auto doc_off = exact(B.doc_off), span_off = exact(B.span_off);
    auto start = exact(B.start), len = exact(B.len);
    std::unique_ptr<uint8_t[]> out(new uint8_t[cap_bytes ? cap_bytes : 1]);
    std::unique_ptr<uint64_t[]> exc_off(new uint64_t[cap_exc + 1]), exc_doc(new uint64_t[cap_exc ? cap_exc : 1]), exc_span_off(new uint64_t[cap_exc + 1]),
        doc_exc_off(new uint64_t[n_docs + 1]);
    std::unique_ptr<uint32_t[]> exc_start(new uint32_t[cap_exc ? cap_exc : 1]), span_rel(new uint32_t[B.start.size() ? B.start.size() : 1]);
    for (size_t s = 0; s < B.start.size(); s++) span_rel[s] = kUntouched;
    uint64_t got_m = ~0ull, got_total = ~0ull;
    const int rc = excerpt_spans_snap_host(text.get(), doc_off.get(), n_docs, span_off.get(), start.get(), len.get(), B.before, B.after, B.flags, B.reach,
                                           word_table_host(), cap_bytes ? out.get() : nullptr, cap_bytes, exc_off.get(),
                                           cap_exc ? exc_doc.get() : nullptr, cap_exc ? exc_start.get() : nullptr, exc_span_off.get(), cap_exc,
                                           B.start.empty() ? nullptr : span_rel.get(), doc_exc_off.get(), &got_m, &got_total);
    expect(rc == GFT_OK, "the walk refuses a good batch", round);
    if (rc != GFT_OK) return;
    expect(got_m == m && got_total == total, "n_exc / total", round);
    if (got_m != m) return;
    for (uint64_t r = 0; r <= m && r <= cap_exc; r++)
        expect(exc_off[r] == want.exc_off[r] && exc_span_off[r] == want.exc_span_off[r], "exc_off / exc_span_off", round);
    for (uint64_t r = 0; r < m && r < cap_exc; r++) expect(exc_doc[r] == want.exc_doc[r] && exc_start[r] == want.exc_start[r], "exc_doc / exc_start", round);
    for (size_t s = 0; s < B.start.size(); s++) expect(span_rel[s] == want.span_rel[s], "span_rel", round);
    for (uint64_t d = 0; d <= n_docs; d++) expect(doc_exc_off[d] == want.doc_exc_off[d], "doc_exc_off", round);
    expect(!std::min(cap_bytes, total) || std::memcmp(out.get(), want.out.data(), (size_t)std::min(cap_bytes, total)) == 0, "the excerpts' bytes", round);
    // no snap bit: the plain walk's answer, whatever the reach
    if (!(B.flags & (GFT_EXCERPT_WORDS | GFT_EXCERPT_LINES)) && cap_bytes == total && cap_exc == m) {
        std::unique_ptr<uint8_t[]> out2(new uint8_t[total ? total : 1]);
        uint64_t m2 = 0, t2 = 0;
        const int rc2 = excerpt_spans_host(text.get(), doc_off.get(), n_docs, span_off.get(), start.get(), len.get(), B.before, B.after, B.flags,
                                           total ? out2.get() : nullptr, total, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, &m2, &t2);
        expect(rc2 == GFT_OK && m2 == m && t2 == total && (!total || std::memcmp(out.get(), out2.get(), (size_t)total) == 0), "no snap bit: not the plain walk",
               round);
    }
}

void check_refused(const Batch& B, uint32_t flags, uint32_t reach, uint64_t round) {
    const uint64_t n_docs = B.doc_off.size() - 1;
    std::vector<uint8_t> out(B.text.size() + 1, 0xA5);
    std::vector<uint64_t> a(B.start.size() + 2, 0xA5A5A5A5A5A5A5A5ull), b(a), c(a), deo(n_docs + 1, 0xA5A5A5A5A5A5A5A5ull);
    std::vector<uint32_t> es(B.start.size() + 1, kUntouched), rel(es);
    uint64_t m = 7, total = 7;
    const int rc = excerpt_spans_snap_host(B.text.data(), B.doc_off.data(), n_docs, B.span_off.data(), B.start.data(), B.len.data(), B.before, B.after, flags,
                                           reach, word_table_host(), out.data(), out.size(), a.data(), b.data(), es.data(), c.data(), B.start.size(),
                                           rel.data(), deo.data(), &m, &total);
    expect(rc == GFT_E_INVALID && m == 0 && total == 0, "a bad call is not refused", round);
    bool clean = true;
    for (uint8_t x : out) clean = clean && x == 0xA5;
    for (auto* v : {&a, &b, &c, &deo})
        for (uint64_t x : *v) clean = clean && x == 0xA5A5A5A5A5A5A5A5ull;
    for (auto* v : {&es, &rel})
        for (uint32_t x : *v) clean = clean && x == kUntouched;
    expect(clean, "a refused call wrote something", round);
}

}  // namespace

int main(int argc, char** argv) {
    const uint64_t rounds = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 100;
    for (uint64_t round = 0; round < rounds; round++) {
        rng.seed(5000 + round);
        Batch B;
        if (round % 10 == 3) B = random_batch(1 + rnd(4), 30, 6, true);                               // words and lines round the greatest reach
        else if (round % 5 == 0) B = random_batch(1 + rnd(12), 400, 3 * kExcTile, false);             // several tiles
        else B = random_batch(1 + rnd(30), 40, 14, false);
        const Result want = brute(B);
        const uint64_t m = want.exc_doc.size(), total = want.out.size();
        check(B, want, total, m, round);
        check(B, want, 0, 0, round);
        if (m) check(B, want, rnd(total + 1), rnd(m), round);
        check_refused(B, GFT_EXCERPT_WORDS | GFT_EXCERPT_LINES, B.reach, round);
        check_refused(B, B.flags | 8u, B.reach, round);
        check_refused(B, B.flags, GFT_EXCERPT_REACH_MAX + 1 + (uint32_t)rnd(100), round);
        if (B.start.size() > B.s0) {                                                                  // a span past its document's end
            Batch bad = B;
            uint64_t d = 0;
            while (B.span_off[d + 1] == B.span_off[d]) d++;
            bad.start[B.span_off[d + 1] - 1] = (uint32_t)(B.doc_off[d + 1] - B.doc_off[d]);
            bad.len[B.span_off[d + 1] - 1] = 1;
            check_refused(bad, B.flags, B.reach, round);
        }
    }
    if (fails) {
        std::fprintf(stderr, "excerpt_snap_check: %d differences\n", fails);
        return 1;
    }
    std::printf("excerpt_snap_check: %llu rounds, walk and brute force agree\n", (unsigned long long)rounds);
    return 0;
}
