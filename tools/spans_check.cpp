// spans_check.cpp -- the span kernels' logic (csrc/gft_spans_piece.hpp, run on the host by hit_spans_host / redact_spans_host) and the
// witness compiler (csrc/witness_terms.cpp) against a brute force written here, under the address and undefined-behaviour
// sanitizers: a stand-alone program, CPU only.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I. tools/spans_check.cpp \
//       gofindthem_amd/csrc/spans_host.cpp gofindthem_amd/csrc/witness_terms.cpp -o build/spans_check
//   build/spans_check 300
//
// Every input and output lies in a heap block of exactly its size -- the match arrays, the rows, the mask, the span arrays of cap
// entries, the text of doc_off[n] bytes --, so a read outside them or a store past a cap is an error of the sanitizer.  N seeded
// random rounds, each: a random set of postfix programs (NOT, INORD, extra slots, repeated slots) compiled into a witness table
// and compared with a recursive evaluation of the definition; a random match CSR with documents of 0 matches and of more than a
// match tile, random rows with ones in their tail bits, every kind of row_idx and mask, filtered by the walk under full caps,
// count only and a cap that cuts the list; the spans of the result, overlapping as they come, masked in a random text by the fill
// walk and by a byte loop; and one span made a byte too long, which must be refused with the text untouched.  The redaction gets
// its spans behind a span base s0 drawn every round, 0 among the values: span_off[0] = s0, the span arrays are blocks of exactly
// s0 + n entries whose first s0 hold a span no document could hold, and the byte loop is indexed the same way.
// Exit code 0: walks and brute force agree everywhere.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <set>
#include <vector>

#include "gofindthem_amd/csrc/gft_spans.hpp"
#include "gofindthem_amd/csrc/witness_terms.hpp"

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

// ---- random programs and the definition of P(i), evaluated on the tree while it is written out --------------------------------
void gen(std::vector<uint32_t>& w, std::set<uint32_t>& wit, uint32_t n_terms, uint32_t n_slots, int depth, bool under_not, bool inord) {
    const uint64_t r = rnd(100);
    const uint32_t fl = inord ? GFT_INORD_FLAG : 0;
    if (depth >= 5 || r < 30) {
        const uint32_t slot = (uint32_t)rnd(n_slots);
        w.push_back(GFT_OP_UNIT << 28 | fl | slot);
        if (!under_not && slot < n_terms) wit.insert(slot);
    } else if (r < 45) {
        gen(w, wit, n_terms, n_slots, depth + 1, true, inord);
        w.push_back(GFT_OP_NOT << 28);
    } else if (r < 52 && !inord) {
        gen(w, wit, n_terms, n_slots, depth + 1, under_not, true);
        w.push_back(GFT_OP_INORD << 28);
    } else {
        gen(w, wit, n_terms, n_slots, depth + 1, under_not, inord);
        gen(w, wit, n_terms, n_slots, depth + 1, under_not, inord);
        w.push_back((r & 1 ? GFT_OP_AND : GFT_OP_OR) << 28 | fl);
    }
}

int fails = 0;
uint64_t runs = 0;
#define CHECK(cond, what)                                                     \
    do {                                                                      \
        if (!(cond)) { fprintf(stderr, "round %d: %s\n", round, what); fails++; return; } \
    } while (0)

void one_round(int round) {
    // ---- the witness table --------------------------------------------------------------------------------------------------
    const uint32_t n_terms = 1 + (uint32_t)rnd(12), n_extra = (uint32_t)rnd(3), n_slots = n_terms + n_extra;
    const uint32_t n_exprs = round % 7 == 0 ? 0 : 1 + (uint32_t)rnd(round % 5 == 0 ? 80 : 40);
    std::vector<uint32_t> words;
    std::vector<uint64_t> poff{0};
    std::vector<std::set<uint32_t>> P(n_exprs);
    for (uint32_t i = 0; i < n_exprs; i++) {
        gen(words, P[i], n_terms, n_slots, 0, false, false);
        poff.push_back(words.size());
    }
    WitnessTable tab;
    {
        auto w = exact(words);
        auto o = exact(poff);
        CHECK(compile_witness_terms(w.get(), o.get(), n_exprs, n_terms, n_slots, tab) == GFT_OK, "the programs were refused");
    }
    CHECK(tab.off.size() == n_terms + 1 && tab.off[0] == 0 && tab.off[n_terms] == tab.expr.size(), "witness offsets");
    for (uint32_t t = 0; t < n_terms; t++) {
        std::vector<uint32_t> want;
        for (uint32_t i = 0; i < n_exprs; i++)
            if (P[i].count(t)) want.push_back(i);
        CHECK(std::vector<uint32_t>(tab.expr.begin() + tab.off[t], tab.expr.begin() + tab.off[t + 1]) == want, "a term's witness list");
    }
    runs++;
    // ---- mark, scan, place ---------------------------------------------------------------------------------------------------
    const uint64_t n_docs = 1 + rnd(40);
    const uint32_t W = (n_exprs + 31) / 32;
    std::vector<uint64_t> moff{0};
    for (uint64_t d = 0; d < n_docs; d++) {
        const uint64_t r = rnd(10);
        moff.push_back(moff.back() + (r < 4 ? 0 : r < 8 ? rnd(6) : r < 9 ? kSpanMarkBlock - 1 + rnd(3) : rnd(3 * kSpanMarkBlock + 6)));
    }
    const uint64_t nm = moff.back();
    std::vector<uint32_t> term(nm), pos(nm), term_len(n_terms);
    for (auto& l : term_len) l = 1 + (uint32_t)rnd(round % 11 == 0 ? 7424 : 9);
    const uint32_t pos_end = round & 1;
    for (uint64_t m = 0; m < nm; m++) {
        term[m] = (uint32_t)rnd(n_terms);
        pos[m] = (pos_end ? term_len[term[m]] - 1 : 0) + (uint32_t)rnd(50);
    }
    const int idx_kind = round % 3;                                 // identity, a permutation of more rows, repeated entries
    const uint64_t n_rows = idx_kind == 0 ? n_docs : idx_kind == 1 ? n_docs + 3 : 1 + n_docs / 2;
    std::vector<uint64_t> row_idx(n_docs);
    for (uint64_t d = 0; d < n_docs; d++) row_idx[d] = idx_kind == 0 ? d : idx_kind == 1 ? (d * 7 + 3) % n_rows : rnd(n_rows);
    const uint32_t tail = (n_exprs & 31) ? ~0u << (n_exprs & 31) : 0u;
    std::vector<uint32_t> rows(n_rows * W), want(W);
    for (auto& w : rows) w = (uint32_t)rng() & (uint32_t)rng() & (round % 4 == 0 ? (uint32_t)rng() : ~0u);
    for (auto& w : want) w = (uint32_t)rng() | (uint32_t)rng();
    for (uint64_t r = 0; W && r < n_rows; r++) rows[r * W + W - 1] |= tail;
    if (W) want[W - 1] |= tail;
    const bool want_null = round % 4 == 1;
    // the contract, one match and one expression at a time
    std::vector<uint64_t> r_off{0};
    std::vector<uint32_t> r_start, r_len, r_term;
    for (uint64_t d = 0; d < n_docs; d++) {
        const uint64_t r = idx_kind == 0 ? d : row_idx[d];
        for (uint64_t m = moff[d]; m < moff[d + 1]; m++) {
            bool kept = false;
            for (uint32_t i = 0; i < n_exprs && !kept; i++)
                kept = P[i].count(term[m]) && (rows[r * W + (i >> 5)] >> (i & 31) & 1) && (want_null || (want[i >> 5] >> (i & 31) & 1));
            if (!kept) continue;
            const uint32_t len = term_len[term[m]];
            r_start.push_back(pos_end ? pos[m] + 1 - len : pos[m]);
            r_len.push_back(len);
            r_term.push_back(term[m]);
        }
        r_off.push_back(r_start.size());
    }
    const uint64_t total = r_start.size();
    auto a_moff = exact(moff);
    auto a_term = exact(term);
    auto a_pos = exact(pos);
    auto a_len = exact(term_len);
    auto a_woff = exact(tab.off);
    auto a_wexp = exact(tab.expr);
    auto a_rows = exact(rows);
    auto a_want = exact(want);
    auto a_idx = exact(row_idx);
    const uint64_t caps[4] = {total, 0, total ? total - 1 : 0, total / 2};
    for (int k = 0; k < 4; k++) {
        const uint64_t cap = caps[k];
        const bool count_only = k == 1;
        std::vector<uint64_t> so(n_docs + 1, ~0ull);
        auto o_off = exact(so);
        auto o_start = exact(std::vector<uint32_t>(cap, ~0u));
        auto o_len = exact(std::vector<uint32_t>(cap, ~0u));
        auto o_term = exact(std::vector<uint32_t>(cap, ~0u));
        uint64_t got = ~0ull;
        const int rc = hit_spans_host(a_moff.get(), a_term.get(), a_pos.get(), n_docs, a_len.get(), pos_end, a_woff.get(), a_wexp.get(), a_rows.get(), n_exprs,
                                      idx_kind == 0 ? nullptr : a_idx.get(), want_null ? nullptr : a_want.get(), count_only ? nullptr : o_off.get(),
                                      cap ? o_start.get() : nullptr, cap && k != 3 ? o_len.get() : nullptr, cap && k != 2 ? o_term.get() : nullptr, cap, &got);
        CHECK(rc == GFT_OK && got == total, "the walk's status or total");
        if (!count_only) CHECK(!memcmp(o_off.get(), r_off.data(), (n_docs + 1) * 8), "span_off");
        for (uint64_t s = 0; s < cap; s++) {
            CHECK(o_start[s] == r_start[s], "span_start");
            if (k != 3) CHECK(o_len[s] == r_len[s], "span_len");
            if (k != 2) CHECK(o_term[s] == r_term[s], "span_term");
        }
        runs++;
    }
    // ---- the redaction of those spans in a random text ----------------------------------------------------------------------------
    const uint64_t lead = rnd(9);
    std::vector<uint64_t> doff{lead};
    for (uint64_t d = 0; d < n_docs; d++) {
        uint64_t need = 0;
        for (uint64_t s = r_off[d]; s < r_off[d + 1]; s++) need = std::max<uint64_t>(need, (uint64_t)r_start[s] + r_len[s]);
        doff.push_back(doff.back() + need + (need && rnd(3) == 0 ? 0 : rnd(5)));        // (a span may end on the document's last byte)
    }
    std::vector<uint8_t> text(doff.back());
    for (auto& b : text) b = (uint8_t)rng();
    std::vector<uint8_t> ref = text;
    const uint32_t mask = (uint32_t)rnd(256);
    // the spans behind a base: [s0, s0 + total) of arrays of exactly s0 + total entries, poison in front
    static const uint64_t base[] = {0, 0, 1, 2, kSpanTile - 1, kSpanTile, kSpanTile + 1, 3 * kSpanTile + 5};
    const uint64_t s0 = rnd(9) < 8 ? base[rnd(8)] : rnd(600);
    std::vector<uint64_t> f_off(r_off);
    for (auto& o : f_off) o += s0;
    std::vector<uint32_t> f_start(s0, 0xFFFFFFFFu), f_len(s0, 0xFFFFFFFFu);
    f_start.insert(f_start.end(), r_start.begin(), r_start.end());
    f_len.insert(f_len.end(), r_len.begin(), r_len.end());
    for (uint64_t d = 0; d < n_docs; d++)
        for (uint64_t s = f_off[d]; s < f_off[d + 1]; s++)
            for (uint32_t j = 0; j < f_len[s]; j++) ref[doff[d] + f_start[s] + j] = (uint8_t)mask;
    auto a_doff = exact(doff);
    auto a_soff = exact(f_off);
    auto a_start = exact(f_start);
    {
        auto a_slen = exact(f_len);
        auto t = exact(text);
        CHECK(redact_spans_host(t.get(), a_doff.get(), n_docs, a_soff.get(), a_start.get(), a_slen.get(), mask) == GFT_OK, "the fill was refused");
        CHECK(!memcmp(t.get(), ref.data(), text.size()), "the masked text");
        CHECK(redact_spans_host(t.get(), a_doff.get(), n_docs, a_soff.get(), a_start.get(), a_slen.get(), 256) == GFT_E_INVALID, "a mask of 256 was taken");
        runs++;
    }
    if (total) {
        // one span made to end a byte behind its document: refused, and no byte of the text changes
        const uint64_t s = rnd(total);
        uint64_t d = 0;
        while (r_off[d + 1] <= s) d++;
        std::vector<uint32_t> bad = f_len;
        bad[s0 + s] = (uint32_t)(doff[d + 1] - doff[d] - r_start[s] + 1);
        auto a_bad = exact(bad);
        auto t = exact(text);
        CHECK(redact_spans_host(t.get(), a_doff.get(), n_docs, a_soff.get(), a_start.get(), a_bad.get(), mask) == GFT_E_INVALID, "a span past its document was taken");
        CHECK(!memcmp(t.get(), text.data(), text.size()), "a refused fill wrote");
        runs++;
    }
    if (s0) {                                                       // span_off[n_docs] < span_off[0]
        std::vector<uint64_t> down(f_off);
        down.back() = s0 - 1;
        auto a_down = exact(down);
        auto a_slen = exact(f_len);
        auto t = exact(text);
        CHECK(redact_spans_host(t.get(), a_doff.get(), n_docs, a_down.get(), a_start.get(), a_slen.get(), mask) == GFT_E_INVALID, "span offsets that descend were taken");
        CHECK(!memcmp(t.get(), text.data(), text.size()), "a refused fill wrote");
        runs++;
    }
}

// the programs the compiler must refuse
void refusals() {
    const int round = -1;
    WitnessTable tab;
    tab.off.assign(1, 77);
    const uint32_t U = GFT_OP_UNIT << 28, A = GFT_OP_AND << 28, N = GFT_OP_NOT << 28;
    const std::vector<std::vector<uint32_t>> bad = {{U, A}, {N}, {U, U | 1}, {}, {U | 5}, {7u << 28}, {U, GFT_OP_INORD << 28, A}};
    for (const auto& p : bad) {
        auto w = exact(p);
        const uint64_t off[2] = {0, p.size()};
        CHECK(compile_witness_terms(w.get(), off, 1, 2, 3, tab) == GFT_E_INVALID && tab.off.size() == 1 && tab.off[0] == 77, "a malformed program was taken");
    }
    const uint64_t down[2] = {1, 0};
    const uint32_t one[1] = {U};
    CHECK(compile_witness_terms(one, down, 1, 2, 3, tab) == GFT_E_INVALID, "descending program offsets were taken");
    runs++;
}

}  // namespace

int main(int argc, char** argv) {
    const int n = argc > 1 ? atoi(argv[1]) : 100;
    refusals();
    for (int round = 0; round < n && !fails; round++) {
        rng.seed(20241019u + (uint64_t)round);
        one_round(round);
    }
    if (fails) { fprintf(stderr, "spans_check: %d failure(s)\n", fails); return 1; }
    printf("spans_check: all cases agree (%llu runs of the walks)\n", (unsigned long long)runs);
    return 0;
}
