// C++ mirror of the reference's group package (group/dsl/*.go, group/finder/finder.go, group/finder/internal.go) on
// top of gft::Finder -- SURVEY.md 8(f) row 2.  Same names, argument meaning and error behaviour; the one structural
// change is the point of the exercise: every string leaf of an object (or of a whole batch of JSON documents) becomes
// one document of ONE Finder::ProcessTexts call, instead of one ProcessText per leaf (internal.go:28-31).
#pragma once
#include <cstdint>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <vector>

#include "finder_host.hpp"
#include "json_mini.hpp"

namespace gft {
namespace gdsl {

// group/dsl/scanner.go:12-35
enum Token { ILLEGAL = 0, END_OF_INPUT, WS, TAG, FIELD_PATH, QUOTATION, OPPAR, CLPAR, AND, OR, NOT };
const char* token_name(Token t);

// group/dsl/expression.go:11-17
enum ExprType { UNSET_EXPR = 0, AND_EXPR, OR_EXPR, NOT_EXPR, UNIT_EXPR };
const char* expr_type_name(ExprType t);

struct TagInfo { std::string Name, FieldPath; };            // expression.go:39-42

struct Expression {                                         // expression.go:46-51
    std::unique_ptr<Expression> LExpr, RExpr;
    ExprType Type = UNSET_EXPR;
    TagInfo Tag;
    mutable int32_t tag_id = -1;                            // batch evaluation: index of Tag.Name among the finder's tags
};

struct ScanResult { Token tok = ILLEGAL; std::string lit; std::string err; };

class Scanner {                                             // scanner.go:67-263
public:
    explicit Scanner(const std::string& src) : s_(src) {}
    ScanResult Scan();
private:
    int32_t read();
    void unread();
    ScanResult scan_whitespace();
    ScanResult scan_operators();
    ScanResult scan_tag();
    ScanResult scan_field_path();
    const std::string& s_;
    size_t i_ = 0, last_ = 0;
};

struct ParseResult {
    std::unique_ptr<Expression> expr;      // null on error
    std::vector<std::string> tags, fields; // unique, first-seen order (GetTags / GetFields, parser.go:281-297)
    std::string err;
};
ParseResult Parse(const std::string& src);                  // parser.go:35-175

// tag -> field path -> set of expression strings (the reference's map[string]map[string]map[string]struct{})
using TagMap = std::map<std::string, std::map<std::string, std::set<std::string>>>;

// Expression.Solve (expression.go:61-125); err = "" when fine
bool Solve(const Expression& e, const TagMap& m, std::string& err);

// the same recursion over a caller-supplied UNIT predicate (batch evaluation keeps tags as ids, not map keys)
template <class UnitPred>
bool SolveWith(const Expression& e, UnitPred&& unit, std::string& err) {
    switch (e.Type) {
    case UNIT_EXPR:
        return unit(e);
    case AND_EXPR:
    case OR_EXPR: {
        if (!e.LExpr || !e.RExpr) {
            err = std::string(e.Type == AND_EXPR ? "AND" : "OR") + " statement do not have right or left expression";
            return false;
        }
        const bool l = SolveWith(*e.LExpr, unit, err);
        if (!err.empty()) return false;
        const bool r = SolveWith(*e.RExpr, unit, err);
        if (!err.empty()) return false;
        return e.Type == AND_EXPR ? (l && r) : (l || r);
    }
    case NOT_EXPR: {
        if (!e.RExpr) { err = "NOT statement do not have expression"; return false; }
        const bool r = SolveWith(*e.RExpr, unit, err);
        if (!err.empty()) return false;
        return !r;
    }
    default:
        err = "unable to process expression type " + std::to_string((int)e.Type);
        return false;
    }
}

std::string ToJson(const Expression& e);                    // {"Type":"AND","LExpr":..,"RExpr":..} / {"Type":"UNIT","Tag":{..}}

}  // namespace gdsl

// group/finder/finder.go:12-17
class GroupFinder {
public:
    struct ExpressionWrapper { std::string ExpressionString; std::unique_ptr<gdsl::Expression> Expression; };
    using RuleResult = std::map<std::string, std::vector<std::string>>;   // expressionsByRule

    explicit GroupFinder(Finder* findthem) : findthem_(findthem) {}
    Error AddRule(const std::string& ruleName, const std::vector<std::string>& expressions);
    std::vector<std::string> GetFieldNames() const { return {fields_.begin(), fields_.end()}; }

    // One entry per input document: err (json.Unmarshal's, or the finder's), else the document's tag map
    // (want_tags) or its rule hits.
    struct DocResult { Error err; gdsl::TagMap tags; RuleResult rules; };
    // ProcessJson / TagJson over a batch (finder.go:80-103,160-172): all string leaves of all documents go through
    // ONE Finder::ProcessTexts; decoding, the walk, rule evaluation run on host threads, a document each
    Error ProcessJsons(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const std::vector<std::string>& includePaths,
                       const std::vector<std::string>& excludePaths, bool want_tags, std::vector<DocResult>& out);
    // EvaluateRules (finder.go:118-137)
    Error EvaluateRules(const gdsl::TagMap& m, RuleResult& out) const;

    // ---- records: a batch of (field, string) leaves under a schema of field paths, rules evaluated on the device
    // (rule_set.hpp, gft_rules.hip).  Every function returns a gft_status and leaves the text of a failure in `err`.
    // Stores the schema after compiling the rules against it: a refusal leaves the previous schema and set answering.
    int SetSchema(const std::vector<std::string>& paths, const std::vector<std::string>& includePaths,
                  const std::vector<std::string>& excludePaths, Error& err);
    // rule expression i in the order of the rule bitmap's bits: ascending rule name, AddRule order inside a name
    struct RuleExpr { const std::string* name; const std::string* expr; };
    const std::vector<RuleExpr>& RuleExprs();
    // device pointers; the leaves go through Finder::ProcessDevice into an engine-owned bitmap, then the two kernels
    int ProcessRecordsDevice(const uint8_t* d_text, const uint64_t* d_leaf_off, const uint32_t* d_leaf_field, const uint64_t* d_rec_off,
                             uint64_t n_records, uint64_t n_leaves, uint32_t* d_rule_bitmap, Error& err);
    // host pointers: upload + ProcessRecordsDevice when the finder qualifies, else Finder::ProcessTexts and the bitmap uploaded
    int ProcessRecords(const uint8_t* text, const uint64_t* leaf_off, const uint32_t* leaf_field, const uint64_t* rec_off, uint64_t n_records,
                       uint64_t n_leaves, uint32_t* rule_bitmap, Error& err);
    // ---- JSON decoded on the device (json_schema.hpp, gft_json.hip) against the schema's trie.  GFT_E_UNSUPPORTED names the
    // trie's limit when the schema is beyond it (SetSchema itself accepts such a schema).
    // device pointers: the record arrays of a batch of raw JSON documents (gft_group_json_leaves_device)
    int JsonLeavesDevice(const uint8_t* d_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint8_t* d_status, uint64_t* d_rec_off,
                         uint32_t* d_leaf_field, uint64_t* d_leaf_off, uint64_t leaf_cap, uint8_t* d_text, uint64_t text_cap, uint64_t* totals,
                         Error& err);
    // ... into engine-owned arrays, then ProcessRecordsDevice: rows of documents with status != 0 are those of an empty record
    int ProcessJsonsDevice(const uint8_t* d_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint8_t* d_status, uint32_t* d_rule_bitmap,
                           Error& err);
    // host pointers: upload, ProcessJsonsDevice, status and rows down; documents the device did not decide go through
    // ProcessJsons as one sub-batch.  The include / exclude lists are the schema's.  A finder that does not qualify for the
    // device record route takes ProcessJsons for the whole batch.  out: as ProcessJsons with want_tags = false.
    int ProcessJsonsSchema(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, std::vector<DocResult>& out, Error& err);
    // ---- the schema discovered from the batch (k_json_paths): what ProcessJson means without SetSchema
    // device pointers: the distinct paths of the batch's string values, sorted bytewise; needs no schema
    int JsonPathsDevice(const uint8_t* d_blob, const uint64_t* d_doc_off, uint64_t n_docs, std::vector<std::string>& paths, uint64_t* dropped,
                        Error& err);
    // host pointers: upload once, discover the paths, compile them into a schema of its own (kept between calls, apart from
    // SetSchema's) and run ProcessJsonsSchema's route on the staged batch.  out: as ProcessJsons with want_tags = false, for
    // every batch; a finder that does not qualify, or a discovered schema beyond a limit, sends the batch through ProcessJsons.
    int ProcessJsonsAuto(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const std::vector<std::string>& includePaths,
                         const std::vector<std::string>& excludePaths, std::vector<DocResult>& out, Error& err);
    // what the last ProcessJsonsAuto found: paths, paths found and not kept, whether it compiled a schema
    uint64_t auto_last_paths = 0, auto_last_dropped = 0, auto_last_recompiled = 0;
    // no device: the reference classification and the kernels' walker on the host (json_schema.hpp), against the stored schema
    int DebugJsonLeaves(bool emulate, const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, uint8_t* status, uint64_t* rec_off,
                        uint32_t* leaf_field, uint64_t* leaf_off, uint64_t leaf_cap, uint8_t* text, uint64_t text_cap, uint64_t* totals, Error& err);
    // the trie's lookup (tests): the child of node `parent` under a component, or `parent` itself for key_len == 0; -1: none.
    // *field: the node's field index, or -1
    int64_t DebugJsonFind(int64_t parent, const uint8_t* key, uint32_t key_len, int64_t* field);
    // documents of the last ProcessJsonsSchema / ProcessJsonsAuto batch decided on the device / handed to ProcessJsons
    uint64_t json_last_device = 0, json_last_host = 0;

    // the compiled device words interpreted on the host over a caller-supplied leaf bitmap: no device
    int DebugEvalRules(const uint32_t* hit_bitmap, uint32_t n_exprs, const uint32_t* leaf_field, const uint64_t* rec_off, uint64_t n_records,
                       uint64_t n_leaves, uint32_t* rule_bitmap, Error& err);

    // the two kernels over a caller-supplied leaf bitmap on the device (the device half of the proof: what the kernels make of
    // rows the finder did not write, bits at and above n_exprs included)
    int DebugEvalRulesDevice(const uint32_t* d_hit_bitmap, uint32_t n_exprs, const uint32_t* d_leaf_field, const uint64_t* d_rec_off,
                             uint64_t n_records, uint64_t n_leaves, uint32_t* d_rule_bitmap, Error& err);

    const std::map<std::string, std::vector<ExpressionWrapper>>& rules() const { return rules_; }
    const std::set<std::string>& fields() const { return fields_; }
    const std::set<std::string>& tags() const { return tags_; }
    // leaves and bytes of the last TagJsons call (measurement)
    uint64_t last_leaves = 0, last_bytes = 0;

private:
    Finder* findthem_;
    std::map<std::string, std::vector<ExpressionWrapper>> rules_;
    std::set<std::string> fields_, tags_;

    struct Records;                        // schema, compiled RuleSet and what it was compiled from (group_host.cpp)
    std::shared_ptr<Records> rec_;
    std::shared_ptr<Records> auto_;        // ProcessJsonsAuto's: stands in for rec_ while that call runs (UseAuto)
    struct UseAuto;
    // ProcessJsonsSchema behind the upload, for whichever schema rec_ is.  Under the caller's RulesLock: ProcessJsonsDevice over
    // the staged batch, status and rows down ...
    int json_staged_rows(gft_engine* e, const uint8_t* d_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint8_t* d_status, uint32_t* d_rows,
                         std::vector<uint8_t>& status, std::vector<uint32_t>& rows, Error& err);
    // ... and behind it: the documents the device did not decide through ProcessJsons as one sub-batch, the others from their rows
    int json_results(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const std::vector<uint8_t>& status,
                     const std::vector<uint32_t>& rows, std::vector<DocResult>& out, Error& err);
    uint64_t rules_version_ = 0;           // counts AddRule calls that changed rules_
    std::vector<RuleExpr> rule_exprs_;
    uint64_t rule_exprs_version_ = ~0ull;
    int compile_current(Error& err);       // the set for the stored schema, redone when rules / finder expressions changed
    int install_current(gft_engine* e, Error& err);
    int json_current(gft_engine* e, Error& err);   // the schema's trie, refused or installed on e (e == nullptr: checked only)
};

// isValidateFieldPath (internal.go:99-119)
bool IsValidFieldPath(const std::string& fieldPath, const std::vector<std::string>& includePaths,
                      const std::vector<std::string>& excludePaths);

}  // namespace gft
