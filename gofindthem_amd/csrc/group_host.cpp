// group_host.cpp -- the reference's GroupFinder (group/finder/finder.go, internal.go): rules in, a batch of JSON documents
// decoded, walked and evaluated on host threads around ONE Finder::ProcessTexts.  See group_host.hpp; the DSL is group_dsl.cpp,
// the device routes are group_records.cpp and group_json.cpp, the C ABI is group_api.cpp.
#include "group_host.hpp"

#include <algorithm>
#include <cstring>
#include <unordered_map>

#include "host_parallel.hpp"

namespace gft {

Error GroupFinder::AddRule(const std::string& ruleName, const std::vector<std::string>& expressions) {   // finder.go:45-66
    for (const auto& raw : expressions) {
        gdsl::ParseResult pr = gdsl::Parse(raw);
        if (!pr.err.empty()) return pr.err;
        ExpressionWrapper w;
        w.ExpressionString = raw;
        w.Expression = std::move(pr.expr);
        rules_[ruleName].push_back(std::move(w));
        rules_version_++;
        for (const auto& t : pr.tags) tags_.insert(t);
        for (const auto& f : pr.fields) fields_.insert(f);
    }
    return "";
}

namespace {
struct Leaf { uint32_t doc; std::string path; const std::string* text; };

// getRulesInfo (internal.go:9-97) over a decoded JSON value: strings are leaves, objects extend the path with
// ".key", arrays with ".index(i)"; numbers, booleans and null are not taggable
void walk(const json::Value& root, const std::string& root_path, uint32_t doc, const std::vector<std::string>& inc,
          const std::vector<std::string>& exc, std::vector<Leaf>& out) {
    // depth first, children in document order, with an explicit stack (documents nest up to 10 000 levels)
    struct Item { const json::Value* v; std::string path; };
    std::vector<Item> todo;
    todo.push_back(Item{&root, root_path});
    while (!todo.empty()) {
        Item it = std::move(todo.back());
        todo.pop_back();
        const json::Value& v = *it.v;
        const std::string& path = it.path;
        switch (v.kind) {
        case json::Value::String:
            if (IsValidFieldPath(path, inc, exc)) out.push_back(Leaf{doc, path, &v.str});
            break;
        case json::Value::Object:
            for (size_t i = v.obj.size(); i-- > 0;) {          // pushed in reverse: popped in document order
                if (!v.last_wins(i)) continue;                   // a Go map keeps the last duplicate
                todo.push_back(Item{&v.obj[i].second, path.empty() ? v.obj[i].first : path + "." + v.obj[i].first});
            }
            break;
        case json::Value::Array:
            for (size_t i = v.arr.size(); i-- > 0;) {
                const std::string fn = "index(" + std::to_string(i) + ")";
                todo.push_back(Item{&v.arr[i], path.empty() ? fn : path + "." + fn});
            }
            break;
        default:
            break;
        }
    }
}

void resolve_tags(const gdsl::Expression& e, const std::unordered_map<std::string, uint32_t>& ids) {
    if (e.Type == gdsl::UNIT_EXPR) { auto it = ids.find(e.Tag.Name); e.tag_id = it == ids.end() ? -1 : (int32_t)it->second; }
    if (e.LExpr) resolve_tags(*e.LExpr, ids);
    if (e.RExpr) resolve_tags(*e.RExpr, ids);
}
}  // namespace

Error GroupFinder::ProcessJsons(const uint8_t* jblob, const uint64_t* doc_off, uint64_t n_docs,
                                const std::vector<std::string>& includePaths, const std::vector<std::string>& excludePaths,
                                bool want_tags, std::vector<DocResult>& out) {
    out.assign(n_docs, DocResult());
    // 1. decode + walk, a document per task
    std::vector<json::Value> docs(n_docs);
    std::vector<std::vector<Leaf>> doc_leaves(n_docs);
    parallel_for(n_docs, [&](uint64_t d, unsigned) {
        out[d].err = json::Parse((const char*)jblob + doc_off[d], (size_t)(doc_off[d + 1] - doc_off[d]), docs[d]);
        if (out[d].err.empty()) walk(docs[d], "", (uint32_t)d, includePaths, excludePaths, doc_leaves[d]);
    });
    // 2. every leaf is one document of one batch
    std::vector<uint64_t> first(n_docs + 1, 0);
    for (uint64_t d = 0; d < n_docs; d++) first[d + 1] = first[d] + doc_leaves[d].size();
    const uint64_t n_leaves = first[n_docs];
    std::vector<uint64_t> off(n_leaves + 1, 0);
    for (uint64_t d = 0; d < n_docs; d++)
        for (size_t k = 0; k < doc_leaves[d].size(); k++) off[first[d] + k + 1] = doc_leaves[d][k].text->size();
    for (uint64_t i = 0; i < n_leaves; i++) off[i + 1] += off[i];
    std::vector<uint8_t> blob(off[n_leaves] + 64, 0);
    parallel_for(n_docs, [&](uint64_t d, unsigned) {
        for (size_t k = 0; k < doc_leaves[d].size(); k++)
            memcpy(blob.data() + off[first[d] + k], doc_leaves[d][k].text->data(), doc_leaves[d][k].text->size());
    });
    last_leaves = n_leaves;
    last_bytes = off[n_leaves];
    const auto& exprs = findthem_->expressions();
    const uint32_t words = (uint32_t)((exprs.size() + 31) / 32);
    std::vector<uint32_t> bitmap((size_t)n_leaves * words + 1, 0);
    if (n_leaves) {
        Error err = findthem_->ProcessTexts(blob.data(), off.data(), n_leaves, bitmap.data());
        if (!err.empty()) {
            // the reference aborts the walk of a document at its first failing ProcessText (internal.go:29-31);
            // the finder's errors (engine build / find, unsolvable expression) do not depend on the text
            for (uint64_t d = 0; d < n_docs; d++)
                if (!doc_leaves[d].empty()) out[d].err = err;
        }
    }
    // 3. bitmap rows -> tags -> rules, a document per task.  Rules only ask "was tag T matched at a path with prefix
    // P" (group/dsl/expression.go:70-82): unless the expression strings are wanted (TagJson) a leaf contributes each of
    // its tags once, and tags are ids rather than map keys
    std::unordered_map<std::string, uint32_t> tag_ids;
    std::vector<uint32_t> tag_of(exprs.size());
    for (size_t e = 0; e < exprs.size(); e++) tag_of[e] = tag_ids.emplace(exprs[e].tag, (uint32_t)tag_ids.size()).first->second;
    const uint32_t n_tags = (uint32_t)tag_ids.size();
    for (const auto& kv : rules_) for (const auto& ew : kv.second) resolve_tags(*ew.Expression, tag_ids);
    struct Scratch { std::vector<std::vector<uint32_t>> leaves_of_tag; std::vector<uint32_t> touched; std::vector<uint8_t> seen; };
    std::vector<Scratch> scratch(host_threads());
    parallel_for(n_docs, [&](uint64_t d, unsigned t) {
        if (!out[d].err.empty()) return;
        const auto& lv = doc_leaves[d];
        if (want_tags) {
            for (size_t k = 0; k < lv.size(); k++) {
                const uint32_t* row = bitmap.data() + (first[d] + k) * words;
                for (uint32_t w = 0; w < words; w++)
                    for (uint32_t bits = row[w]; bits; bits &= bits - 1) {
                        const uint32_t e = w * 32 + (uint32_t)__builtin_ctz(bits);
                        out[d].tags[exprs[e].tag][lv[k].path].insert(exprs[e].exprString);
                    }
            }
            return;
        }
        Scratch& sc = scratch[t];
        if (sc.leaves_of_tag.size() != n_tags) { sc.leaves_of_tag.assign(n_tags, {}); sc.seen.assign(n_tags, 0); }
        for (uint32_t tg : sc.touched) sc.leaves_of_tag[tg].clear();
        sc.touched.clear();
        for (size_t k = 0; k < lv.size(); k++) {
            const uint32_t* row = bitmap.data() + (first[d] + k) * words;
            std::fill(sc.seen.begin(), sc.seen.end(), 0);
            for (uint32_t w = 0; w < words; w++)
                for (uint32_t bits = row[w]; bits; bits &= bits - 1) {
                    const uint32_t tg = tag_of[w * 32 + (uint32_t)__builtin_ctz(bits)];
                    if (sc.seen[tg]) continue;
                    sc.seen[tg] = 1;
                    if (sc.leaves_of_tag[tg].empty()) sc.touched.push_back(tg);
                    sc.leaves_of_tag[tg].push_back((uint32_t)k);
                }
        }
        auto unit = [&](const gdsl::Expression& u) {
            if (u.tag_id < 0) return false;
            const auto& where = sc.leaves_of_tag[u.tag_id];
            if (where.empty()) return false;
            if (u.Tag.FieldPath.empty()) return true;
            for (uint32_t k : where)
                if (lv[k].path.compare(0, u.Tag.FieldPath.size(), u.Tag.FieldPath) == 0) return true;
            return false;
        };
        for (const auto& kv : rules_)
            for (const auto& ew : kv.second) {
                std::string err;
                const bool v = gdsl::SolveWith(*ew.Expression, unit, err);
                if (!err.empty()) { out[d].err = err; out[d].rules.clear(); return; }
                if (v) out[d].rules[kv.first].push_back(ew.ExpressionString);
            }
    });
    return "";
}

Error GroupFinder::EvaluateRules(const gdsl::TagMap& m, RuleResult& out) const {    // finder.go:118-137
    out.clear();
    for (const auto& kv : rules_)
        for (const auto& ew : kv.second) {
            std::string err;
            const bool v = gdsl::Solve(*ew.Expression, m, err);
            if (!err.empty()) { out.clear(); return err; }
            if (v) out[kv.first].push_back(ew.ExpressionString);
        }
    return "";
}

const std::vector<GroupFinder::RuleExpr>& GroupFinder::RuleExprs() {
    if (rule_exprs_version_ != rules_version_) {
        rule_exprs_.clear();
        for (const auto& kv : rules_)
            for (const auto& ew : kv.second) rule_exprs_.push_back(RuleExpr{&kv.first, &ew.ExpressionString});
        rule_exprs_version_ = rules_version_;
    }
    return rule_exprs_;
}

}  // namespace gft
