// rules_json_check.cpp -- make_rule_fragments and rules_json_host (csrc/rules_json.cpp: the fragment table and the host statement
// of the result kernels' contract) under the address and undefined-behaviour sanitizers: a stand-alone program, CPU only.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I. tools/rules_json_check.cpp \
//       gofindthem_amd/csrc/rules_json.cpp gofindthem_amd/csrc/dsl_compile.cpp -o build/rules_json_check
//   build/rules_json_check 3000 1
//
// N seeded rule sets and batches.  Names and expressions are arbitrary byte strings -- make_rule_fragments takes what AddRule
// would refuse, so fragments of 2 and 3 bytes (an empty and a one-byte expression) occur beside those of 63 .. 257 and 5 000
// bytes --; rules have 1 .. 70 expressions and lie anywhere across the word borders.  Every array -- the five columns of the
// table, the blob with its slack, rows, hole lengths, offsets, the text -- lies in a heap block of exactly its size, so that a
// read or a store past an end is an error of the sanitizer.  Every batch runs with caps 0, 1, 11, 12, total - 1, total, total + 7
// and one in the middle, with and without holes (and with every document a hole), and is compared with a restatement that builds
// the documents with strings.  Exit code 0: all agree.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "gofindthem_amd/csrc/rules_json.hpp"

using namespace gft;

namespace {

template <class T>
std::unique_ptr<T[]> exact(const std::vector<T>& v) {
    std::unique_ptr<T[]> p(new T[v.size()]);
    if (!v.empty()) memcpy(p.get(), v.data(), v.size() * sizeof(T));
    return p;
}

// the escaper, restated: json_str's cases one by one
std::string quoted(const std::string& s) {
    static const char* hex = "0123456789abcdef";
    std::string o = "\"";
    for (unsigned char c : s) {
        switch (c) {
            case '"': o += "\\\""; break;
            case '\\': o += "\\\\"; break;
            case '\n': o += "\\n"; break;
            case '\r': o += "\\r"; break;
            case '\t': o += "\\t"; break;
            default:
                if (c < 0x20) { o += "\\u00"; o += hex[c >> 4]; o += hex[c & 15]; }
                else o += (char)c;
        }
    }
    return o + "\"";
}

std::string random_bytes(std::mt19937_64& rng, size_t n) {
    static const unsigned char kPool[] = {'a', 'z', '"', '\\', '\n', '\r', '\t', 0x01, 0x1f, 0x7f, 0xc3, 0xa9, 0xff, ' ', ':', 0};
    std::string s;
    for (size_t k = 0; k < n; k++) s += (char)kPool[rng() % sizeof kPool];
    return s;
}

struct Set {
    std::vector<std::string> names, exprs;        // [R], a rule's expressions contiguous, names ascending
    std::vector<uint32_t> rule_of;                // [R]
};

Set make_set(std::mt19937_64& rng) {
    static const uint32_t kR[] = {0, 1, 31, 32, 33, 64, 65, 200, 2049};
    static const size_t kLen[] = {0, 1, 2, 3, 57, 58, 59, 249, 250, 251, 4994};
    Set s;
    const uint32_t R = kR[rng() % 9];
    uint32_t rule = 0;
    while (s.exprs.size() < R) {
        static const uint32_t kSize[] = {1, 1, 2, 3, 20, 31, 33, 70};
        const uint32_t size = std::min<uint32_t>(kSize[rng() % 8], R - (uint32_t)s.exprs.size());
        char head[16];
        snprintf(head, sizeof head, "%06u", rule);                 // (distinct and ascending, whatever bytes follow; the first rule's name may be empty)
        const std::string name = (rule ? std::string(head) : std::string()) + random_bytes(rng, rng() % 4 ? rng() % 6 : kLen[rng() % 11]);
        for (uint32_t k = 0; k < size; k++) {
            s.names.push_back(name);
            s.exprs.push_back(random_bytes(rng, rng() % 32 ? rng() % 12 : kLen[rng() % 11]));
            s.rule_of.push_back(rule);
        }
        rule++;
    }
    return s;
}

bool check(const Set& s, std::mt19937_64& rng, uint64_t& bytes, uint64_t& hole_docs) {
    const uint32_t R = (uint32_t)s.exprs.size();
    const uint64_t RW = (R + 31) / 32;
    std::vector<GroupFinder::RuleExpr> exprs;
    for (uint32_t i = 0; i < R; i++) exprs.push_back(GroupFinder::RuleExpr{&s.names[i], &s.exprs[i]});
    RuleFragments built;
    std::string why;
    if (!make_rule_fragments(exprs, built, why)) return false;
    // the table in blocks of exactly its size
    RuleFragments fr;
    fr.rule_first = built.rule_first; fr.name_off = built.name_off; fr.name_len = built.name_len;
    fr.expr_off = built.expr_off; fr.expr_len = built.expr_len; fr.blob = built.blob;
    for (auto* v : {&fr.rule_first, &fr.name_off, &fr.name_len, &fr.expr_off, &fr.expr_len}) v->shrink_to_fit();
    fr.blob.shrink_to_fit();
    if (fr.blob.size() < kRuleFragSlack) return false;
    for (uint32_t i = 0; i < R; i++) {
        const std::string n = quoted(s.names[i]) + ":[", e = quoted(s.exprs[i]);
        if (fr.name_len[i] != n.size() || fr.expr_len[i] != e.size()) return false;
        if (memcmp(fr.blob.data() + fr.name_off[i], n.data(), n.size()) || memcmp(fr.blob.data() + fr.expr_off[i], e.data(), e.size())) return false;
        if (fr.rule_first[i] > i || s.rule_of[fr.rule_first[i]] != s.rule_of[i] || (fr.rule_first[i] && s.rule_of[fr.rule_first[i] - 1] == s.rule_of[i])) return false;
    }
    static const uint64_t kDocs[] = {0, 1, 2, 5, 63, 64, 65, 129};
    const uint64_t n_docs = kDocs[rng() % (R > 100 ? 4 : 8)];             // (the widest rows: a few documents)
    std::vector<uint32_t> rows;
    for (uint64_t d = 0; d < n_docs; d++) {
        const unsigned density = rng() % 5;               // empty, sparse, one bit a word, half, every bit (garbage above R included)
        for (uint64_t w = 0; w < RW; w++) {
            const uint32_t x = (uint32_t)rng(), y = (uint32_t)rng();
            rows.push_back(density == 0 ? 0u : density == 1 ? (x & y & (uint32_t)rng()) : density == 2 ? 1u << (x & 31) : density == 3 ? x : 0xFFFFFFFFu);
        }
    }
    auto d_rows = exact(rows);
    for (int hole_mode = 0; hole_mode < 3; hole_mode++) {  // none, some (first, last, adjacent), every document
        std::vector<uint64_t> holes(n_docs, 0);
        for (uint64_t d = 0; d < n_docs; d++)
            if (hole_mode == 2 || (hole_mode == 1 && (d == 0 || d + 1 == n_docs || d == n_docs / 2 || d == n_docs / 2 + 1 || rng() % 7 == 0))) holes[d] = 12 + rng() % 90;
        // the restatement: strings
        std::string want = "[";
        std::vector<uint64_t> want_off{1};
        for (uint64_t d = 0; d < n_docs; d++) {
            std::string doc;
            if (holes[d]) {
                doc.assign((size_t)holes[d], (char)0xA5);
                hole_docs++;
            } else {
                doc = "{\"rules\":{";
                int64_t open_rule = -1;
                for (uint32_t i = 0; i < R; i++) {
                    if (!((rows[d * RW + i / 32] >> (i % 32)) & 1)) continue;
                    if (open_rule == (int64_t)s.rule_of[i]) doc += ",";
                    else { if (open_rule >= 0) doc += "],"; doc += quoted(s.names[i]) + ":["; open_rule = s.rule_of[i]; }
                    doc += quoted(s.exprs[i]);
                }
                if (open_rule >= 0) doc += "]";
                doc += "}}";
            }
            if (d) want += ",";
            want += doc;
            want_off.push_back(want.size() + 1);
        }
        want += "]";
        const uint64_t total = want.size();
        bytes += total;
        auto d_holes = exact(holes);
        const uint64_t caps[8] = {0, 1, 11, 12, total - 1, total, total + 7, total / 2};
        for (uint64_t cap : caps) {
            std::unique_ptr<uint64_t[]> out_off(new uint64_t[n_docs + 1]);
            std::unique_ptr<uint8_t[]> out(new uint8_t[cap]);
            memset(out.get(), 0xA5, cap);
            uint64_t got_total = ~0ull;
            if (!rules_json_host(fr, d_rows.get(), n_docs, hole_mode ? d_holes.get() : nullptr, cap ? out.get() : nullptr, cap, out_off.get(), &got_total)) return false;
            if (got_total != total || memcmp(out_off.get(), want_off.data(), (n_docs + 1) * 8)) return false;
            for (uint64_t k = 0; k < cap; k++)
                if (out[k] != (k < total ? (uint8_t)want[k] : 0xA5)) return false;
        }
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    const uint64_t n = argc > 1 ? strtoull(argv[1], nullptr, 10) : 3000;
    std::mt19937_64 rng(argc > 2 ? strtoull(argv[2], nullptr, 10) : 1);
    uint64_t bytes = 0, hole_docs = 0, short_frags = 0;
    for (uint64_t i = 0; i < n; i++) {
        const Set s = make_set(rng);
        for (const auto& e : s.exprs) short_frags += e.size() <= 1;
        if (!check(s, rng, bytes, hole_docs)) { fprintf(stderr, "batch %llu: rules_json_host disagrees with the restatement\n", (unsigned long long)i); return 1; }
    }
    // a refusal: a hole the 32-bit counts cannot hold
    {
        RuleFragments fr;
        std::string why;
        if (!make_rule_fragments({}, fr, why)) return 1;
        uint64_t hole = 1ull << 32, off[2], total = 0;
        if (rules_json_host(fr, nullptr, 1, &hole, nullptr, 0, off, &total)) { fprintf(stderr, "a hole of 4 GiB was accepted\n"); return 1; }
    }
    printf("rules_json_check: %llu batches, %llu bytes of text, %llu holes, %llu fragments of 2 or 3 bytes: ok\n", (unsigned long long)n,
           (unsigned long long)bytes, (unsigned long long)hole_docs, (unsigned long long)short_frags);
    return bytes && hole_docs && short_frags ? 0 : 2;    // (a run without text, holes or the shortest fragments checked too little)
}
