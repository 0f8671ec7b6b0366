// rules_json.cpp -- make_rule_fragments, rules_json_host, rule_doc_text (rules_json.hpp): a bit at a time, a byte at a time.
#include "rules_json.hpp"

#include "dsl_compile.hpp"

namespace gft {

bool make_rule_fragments(const std::vector<GroupFinder::RuleExpr>& exprs, RuleFragments& out, std::string& why) {
    out = RuleFragments();
    std::string blob, frag;
    // the longest document -- every bit set -- is the blob plus at most 3 bytes a bit and the frame; it and its separator are
    // one 32-bit count on the device
    const uint64_t limit = 0xFFFFFFFFull - 3 * (uint64_t)exprs.size() - kRuleDocFixed - 2;
    for (size_t i = 0; i < exprs.size(); i++) {
        const bool first = i == 0 || *exprs[i].name != *exprs[i - 1].name;
        if (first) {
            frag.clear();
            dsl::json_str(*exprs[i].name, frag);
            frag += ":[";
            out.name_off.push_back((uint32_t)blob.size());
            out.name_len.push_back((uint32_t)frag.size());
            out.rule_first.push_back((uint32_t)i);
            blob += frag;
        } else {
            out.name_off.push_back(out.name_off.back());
            out.name_len.push_back(out.name_len.back());
            out.rule_first.push_back(out.rule_first.back());
        }
        frag.clear();
        dsl::json_str(*exprs[i].expr, frag);
        out.expr_off.push_back((uint32_t)blob.size());
        out.expr_len.push_back((uint32_t)frag.size());
        blob += frag;
        if (blob.size() > limit) {
            out = RuleFragments();
            why = "the rule names and expressions, escaped, do not fit 32-bit offsets";
            return false;
        }
    }
    out.blob.assign(blob.begin(), blob.end());
    out.blob.resize(blob.size() + kRuleFragSlack, 0);
    return true;
}

namespace {

// the stores of one batch: a byte at a position at or past the cap is dropped
struct CappedText {
    uint8_t* out; uint64_t cap;
    void put(uint64_t at, uint8_t c) const { if (at < cap) out[at] = c; }
    void put(uint64_t at, const uint8_t* p, uint64_t n) const { for (uint64_t k = 0; k < n; k++) put(at + k, p[k]); }
    void put(uint64_t at, const char* s) const { for (; *s; s++, at++) put(at, (uint8_t)*s); }
};

}  // namespace

bool rules_json_host(const RuleFragments& fr, const uint32_t* rule_bitmap, uint64_t n_docs, const uint64_t* hole_len, uint8_t* out, uint64_t cap,
                     uint64_t* out_off, uint64_t* total) {
    const uint32_t R = fr.n_exprs();
    const uint64_t RW = (R + 31) / 32;
    const CappedText T{out, out ? cap : 0};
    if (hole_len)
        for (uint64_t d = 0; d < n_docs; d++)
            if (hole_len[d] >= 0xFFFFFFFFull) return false;
    uint64_t at = 1;
    T.put(0, '[');
    out_off[0] = 1;
    for (uint64_t d = 0; d < n_docs; d++) {
        if (hole_len && hole_len[d]) {
            at += hole_len[d];
        } else {
            const uint32_t* row = rule_bitmap + d * RW;
            T.put(at, "{\"rules\":{");
            at += 10;
            int64_t prev = -1;                            // the set bit before this one
            for (uint32_t i = 0; i < R; i++) {
                if (!row[i >> 5]) { i |= 31; continue; }
                if (!(row[i >> 5] >> (i & 31) & 1u)) continue;
                if (prev < (int64_t)fr.rule_first[i]) {   // the first true expression of its rule
                    if (prev >= 0) { T.put(at, "],"); at += 2; }
                    T.put(at, fr.blob.data() + fr.name_off[i], fr.name_len[i]);
                    at += fr.name_len[i];
                } else {
                    T.put(at++, ',');
                }
                T.put(at, fr.blob.data() + fr.expr_off[i], fr.expr_len[i]);
                at += fr.expr_len[i];
                prev = i;
            }
            if (prev >= 0) T.put(at++, ']');
            T.put(at, "}}");
            at += 2;
        }
        T.put(at++, d + 1 == n_docs ? ']' : ',');
        out_off[d + 1] = at;
    }
    if (!n_docs) T.put(at++, ']');
    if (total) *total = at;
    return true;
}

void rule_doc_text(const std::string& err, const std::map<std::string, std::vector<std::string>>& rules, std::string& o) {
    if (!err.empty()) { o += "{\"error\":"; dsl::json_str(err, o); o += "}"; return; }
    o += "{\"rules\":{";
    bool first = true;
    for (const auto& kv : rules) {
        if (!first) o += ",";
        first = false;
        dsl::json_str(kv.first, o);
        o += ":[";
        for (size_t i = 0; i < kv.second.size(); i++) { if (i) o += ","; dsl::json_str(kv.second[i], o); }
        o += "]";
    }
    o += "}}";
}

}  // namespace gft
