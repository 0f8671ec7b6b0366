// rule_set.cpp -- see rule_set.hpp
#include "rule_set.hpp"

#include <algorithm>
#include <map>
#include <unordered_map>

namespace gft {

namespace {

struct Compiler {
    const std::vector<std::string>& schema;
    const std::unordered_map<std::string, uint32_t>& tag_id;
    RuleSet& rs;
    std::unordered_map<std::string, uint32_t> mask_of;          // prefix -> mask id
    std::map<std::pair<uint32_t, uint32_t>, uint32_t> unit_of;  // (tag id, mask id) -> unit
    std::string err;
    int code = GFT_OK;

    uint32_t mask(const std::string& prefix) {
        auto it = mask_of.find(prefix);
        if (it != mask_of.end()) return it->second;
        const uint32_t id = (uint32_t)rs.prefixes.size();
        rs.prefixes.push_back(prefix);
        for (uint32_t w = 0; w < rs.field_words; w++) {
            uint32_t bits = 0;
            for (uint32_t b = 0; b < 32 && w * 32 + b < rs.n_fields; b++)      // strings.HasPrefix: a plain byte prefix
                if (schema[w * 32 + b].compare(0, prefix.size(), prefix) == 0) bits |= 1u << b;
            rs.masks.push_back(bits & rs.valid[w]);
        }
        mask_of.emplace(prefix, id);
        return id;
    }

    uint32_t unit(const gdsl::TagInfo& t) {
        auto it = tag_id.find(t.Name);
        const uint32_t tg = it == tag_id.end() ? kRuleNoTag : it->second;    // (the reference's map lookup misses)
        const auto key = std::make_pair(tg, mask(t.FieldPath));
        auto u = unit_of.find(key);
        if (u != unit_of.end()) return u->second;
        const uint32_t id = rs.n_units();
        rs.units.push_back(key.first);
        rs.units.push_back(key.second);
        unit_of.emplace(key, id);
        return id;
    }

    // postfix of e behind rs.prog; returns its operand-stack depth (0 after a refusal).  The recursion is as deep as the
    // parser's own (Parse recursed through the same parentheses)
    uint32_t emit(const gdsl::Expression& e) {
        switch (e.Type) {
        case gdsl::UNIT_EXPR:
            rs.prog.push_back(kRopUnit << 28 | unit(e.Tag));
            return 1;
        case gdsl::AND_EXPR:
        case gdsl::OR_EXPR: {
            if (!e.LExpr || !e.RExpr)
                return refuse(GFT_E_ENGINE, std::string(e.Type == gdsl::AND_EXPR ? "AND" : "OR") + " statement do not have right or left expression");
            const uint32_t l = emit(*e.LExpr);
            if (code) return 0;
            const uint32_t r = emit(*e.RExpr);
            if (code) return 0;
            rs.prog.push_back((e.Type == gdsl::AND_EXPR ? kRopAnd : kRopOr) << 28);
            return std::max(l, r + 1);
        }
        case gdsl::NOT_EXPR: {
            if (!e.RExpr) return refuse(GFT_E_ENGINE, "NOT statement do not have expression");
            const uint32_t r = emit(*e.RExpr);
            if (code) return 0;
            rs.prog.push_back(kRopNot << 28);
            return r;
        }
        default:
            return refuse(GFT_E_ENGINE, "unable to process expression type " + std::to_string((int)e.Type));
        }
    }
    uint32_t refuse(int c, const std::string& msg) { code = c; err = msg; return 0; }
};

inline bool bit(const uint32_t* row, uint32_t i) { return row[i >> 5] >> (i & 31) & 1; }

}  // namespace

int compile_rules(const RuleMap& rules, const std::vector<std::string>& tags,
                  const std::vector<uint32_t>& expr_tag, const std::vector<std::string>& schema,
                  const std::vector<std::string>& includePaths, const std::vector<std::string>& excludePaths, RuleSet& out, std::string& err) {
    if (schema.size() > kRuleMaxFields) {
        err = "record schema: " + std::to_string(schema.size()) + " fields, the device form takes at most " + std::to_string(kRuleMaxFields);
        return GFT_E_UNSUPPORTED;
    }
    for (uint32_t t : expr_tag)
        if (t >= tags.size()) { err = "record rules: an expression's tag id is not among the finder's tags"; return GFT_E_INTERNAL; }
    RuleSet rs;
    rs.n_fields = (uint32_t)schema.size();
    rs.n_tags = (uint32_t)tags.size();
    rs.n_exprs = (uint32_t)expr_tag.size();
    rs.expr_tag = expr_tag;
    rs.field_words = (rs.n_fields + 31) / 32;
    rs.valid.assign(rs.field_words, 0);
    for (uint32_t f = 0; f < rs.n_fields; f++)
        if (IsValidFieldPath(schema[f], includePaths, excludePaths)) rs.valid[f >> 5] |= 1u << (f & 31);
    std::unordered_map<std::string, uint32_t> tag_id;
    for (uint32_t t = 0; t < rs.n_tags; t++) tag_id.emplace(tags[t], t);
    Compiler c{schema, tag_id, rs, {}, {}, "", GFT_OK};
    rs.prog_off.push_back(0);
    for (const auto& kv : rules)
        for (const auto& ew : kv.second) {
            const uint32_t d = c.emit(*ew.Expression);
            if (c.code) { err = c.err; return c.code; }
            if (d > kRuleMaxDepth) {
                err = "record rules: rule '" + kv.first + "' expression " + ew.ExpressionString + " needs an operand stack of " + std::to_string(d) +
                      ", the device form takes at most " + std::to_string(kRuleMaxDepth);
                return GFT_E_UNSUPPORTED;
            }
            if (rs.n_units() > kRuleMaxUnits) {
                err = "record rules: more than " + std::to_string(kRuleMaxUnits) + " distinct (tag, field path) units";
                return GFT_E_UNSUPPORTED;
            }
            rs.depth.push_back(d);
            rs.max_depth = std::max(rs.max_depth, d);
            rs.prog_off.push_back((uint32_t)rs.prog.size());
        }
    rs.n_rules = (uint32_t)rs.depth.size();
    out = std::move(rs);
    return GFT_OK;
}

std::string validate_records(uint32_t n_fields, const uint32_t* leaf_field, const uint64_t* rec_off, uint64_t n_records, uint64_t n_leaves) {
    if (!n_records) return n_leaves ? "record batch: leaves but no records" : "";
    if (!rec_off) return "record batch: no record offsets";
    if (n_leaves && !leaf_field) return "record batch: no field indices";
    for (uint64_t r = 0; r < n_records; r++)
        if (rec_off[r] > rec_off[r + 1]) return "record batch: rec_off descends at record " + std::to_string(r);
    if (rec_off[n_records] != n_leaves) return "record batch: rec_off does not end at n_leaves";
    for (uint64_t l = 0; l < n_leaves; l++)
        if (leaf_field[l] >= n_fields)
            return "record batch: leaf " + std::to_string(l) + " names field " + std::to_string(leaf_field[l]) + " of a schema of " + std::to_string(n_fields);
    return "";
}

void eval_rules_host(const RuleSet& rs, const uint32_t* hit_bitmap, const uint32_t* leaf_field, const uint64_t* rec_off, uint64_t n_records,
                     uint32_t* rule_bitmap) {
    const uint32_t EW = (rs.n_exprs + 31) / 32, TW = (rs.n_tags + 31) / 32, RW = (rs.n_rules + 31) / 32, U = rs.n_units();
    std::vector<uint32_t> tag_row(TW);
    std::vector<uint8_t> unit(U);
    std::vector<uint8_t> stack(rs.max_depth + 1);
    for (uint64_t r = 0; r < n_records; r++) {
        std::fill(unit.begin(), unit.end(), 0);
        for (uint64_t l = rec_off[r]; l < rec_off[r + 1]; l++) {
            // k_leaf_tags: bits at and above n_exprs in the row's last word are not read
            std::fill(tag_row.begin(), tag_row.end(), 0);
            const uint32_t* hit = hit_bitmap + l * EW;
            for (uint32_t x = 0; x < rs.n_exprs; x++)
                if (bit(hit, x)) tag_row[rs.expr_tag[x] >> 5] |= 1u << (rs.expr_tag[x] & 31);
            // k_record_rules, phase 1
            const uint32_t f = leaf_field[l];
            for (uint32_t u = 0; u < U; u++) {
                const uint32_t tg = rs.units[2 * u], m = rs.units[2 * u + 1];
                if (tg != kRuleNoTag && bit(rs.masks.data() + (size_t)m * rs.field_words, f) && bit(tag_row.data(), tg)) unit[u] = 1;
            }
        }
        uint32_t* row = rule_bitmap + r * RW;
        std::fill(row, row + RW, 0u);
        for (uint32_t k = 0; k < rs.n_rules; k++) {         // phase 2
            uint32_t sp = 0;
            for (uint32_t i = rs.prog_off[k]; i < rs.prog_off[k + 1]; i++) {
                const uint32_t w = rs.prog[i];
                switch (w >> 28) {
                case kRopUnit: stack[sp++] = unit[w & 0x0FFFFFFFu]; break;
                case kRopAnd: sp--; stack[sp - 1] &= stack[sp]; break;
                case kRopOr: sp--; stack[sp - 1] |= stack[sp]; break;
                default: stack[sp - 1] ^= 1; break;
                }
            }
            if (stack[0]) row[k >> 5] |= 1u << (k & 31);
        }
    }
}

}  // namespace gft
