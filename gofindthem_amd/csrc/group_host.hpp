// C++ mirror of the reference's group package (group/dsl/*.go, group/finder/finder.go, group/finder/internal.go) on
// top of gft::Finder -- SURVEY.md 8(f) row 2.  Same names, argument meaning and error behaviour; the one structural
// change is the point of the exercise: every string leaf of an object (or of a whole batch of JSON documents) becomes
// one document of ONE Finder::ProcessTexts call, instead of one ProcessText per leaf (internal.go:28-31).
#pragma once
#include <cstdint>
#include <functional>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <vector>

#include "finder_host.hpp"
#include "group_dsl.hpp"
#include "json_mini.hpp"

namespace gft {

struct RuleFragments;                      // rules_json.hpp
struct TagSlots;                           // tags_json.hpp
struct TagFields;

// group/finder/finder.go:12-17
class GroupFinder {
public:
    using ExpressionWrapper = gft::ExpressionWrapper;
    using RuleResult = std::map<std::string, std::vector<std::string>>;   // expressionsByRule

    explicit GroupFinder(Finder* findthem) : findthem_(findthem), device_result_(env_device_result()) {}
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
    // text != nullptr: the caller wants the result document ('[' D0 ',' D1 ... ']', rules_json.hpp).  When the device route answers
    // and writes it (gft_result.hip), text->written is set, the rows never cross the link and `out` stays empty; otherwise `out`
    // is filled as without it and the caller serialises.
    struct ResultText { std::string* text = nullptr; bool written = false; };
    int ProcessJsonsSchema(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, std::vector<DocResult>& out, Error& err,
                           ResultText* text = nullptr);
    // ---- the schema discovered from the batch (k_json_paths): what ProcessJson means without SetSchema
    // device pointers: the distinct paths of the batch's string values, sorted bytewise; needs no schema
    int JsonPathsDevice(const uint8_t* d_blob, const uint64_t* d_doc_off, uint64_t n_docs, std::vector<std::string>& paths, uint64_t* dropped,
                        Error& err);
    // host pointers: upload once, discover the paths, compile them into a schema of its own (kept between calls, apart from
    // SetSchema's) and run ProcessJsonsSchema's route on the staged batch.  out: as ProcessJsons with want_tags = false, for
    // every batch; a finder that does not qualify, or a discovered schema beyond a limit, sends the batch through ProcessJsons.
    int ProcessJsonsAuto(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const std::vector<std::string>& includePaths,
                         const std::vector<std::string>& excludePaths, std::vector<DocResult>& out, Error& err, ResultText* text = nullptr);
    // host pointers, JSON Lines: the blob is uploaded once and cut into documents where it lies (gft_split_lines_device,
    // GFT_SPLIT_JSON_LINES), the offsets come down, and ProcessJsonsSchema's route (a schema is set: the lists must be empty,
    // GFT_E_INVALID otherwise) or ProcessJsonsAuto's (none is set) continues from the resident blob.  A finder that does not
    // qualify splits on the host (split_lines_host) and takes ProcessJsons.
    int ProcessJsonLines(const uint8_t* blob, uint64_t len, const std::vector<std::string>& includePaths,
                         const std::vector<std::string>& excludePaths, std::vector<DocResult>& out, Error& err, ResultText* text = nullptr);
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

    // ---- the result document of rule rows as text (rules_json.hpp, gft_result.hip): depends on the rules only, not on a schema.
    // device pointers except total: rows [n_docs][ceil(R / 32)] as ProcessJsonsDevice / ProcessRecordsDevice leave them -> text
    // and out_off [n_docs + 1] under the cap protocol; d_hole_len nullable.  GFT_E_UNSUPPORTED: rules whose fragment table the
    // format cannot hold
    int RulesJsonDevice(const uint32_t* d_rule_bitmap, uint64_t n_docs, const uint64_t* d_hole_len, uint8_t* d_out, uint64_t cap,
                        uint64_t* d_out_off, uint64_t* total, Error& err);
    // rules_json_host over the group's current rules: no device, no schema
    int DebugRulesJson(const uint32_t* rule_bitmap, uint64_t n_docs, const uint64_t* hole_len, uint8_t* out, uint64_t cap, uint64_t* out_off,
                       uint64_t* total, Error& err);

    // ---- tag entries: TagObject's map of every record as a sparse list of (field, expression) pairs (gft_tags.hip, include/gft.h).
    // The arrays of one result; device pointers in the *Device calls (total is always host memory)
    struct TagEntries { uint64_t* row_off; uint32_t* ent_field; uint32_t* ent_expr; uint32_t* ent_tag; uint64_t cap; uint64_t* total; };
    // device pointers; the leaves go through Finder::ProcessDevice into the engine's leaf bitmap, then the three launches
    int TagRecordsDevice(const uint8_t* d_text, const uint64_t* d_leaf_off, const uint32_t* d_leaf_field, const uint64_t* d_rec_off,
                         uint64_t n_records, uint64_t n_leaves, const TagEntries& d_out, Error& err);
    // host pointers: upload + the call above + the arrays down when the finder qualifies, else Finder::ProcessTexts and
    // tag_entries_host; both routes give the same arrays
    int TagRecords(const uint8_t* text, const uint64_t* leaf_off, const uint32_t* leaf_field, const uint64_t* rec_off, uint64_t n_records,
                   uint64_t n_leaves, const TagEntries& out, Error& err);
    // device pointers: JsonLeavesDevice into engine-owned arrays, then TagRecordsDevice; a document with status != 0 has an empty row
    int TagJsonsDevice(const uint8_t* d_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint8_t* d_status, const TagEntries& d_out, Error& err);
    // ProcessJsonsSchema / ProcessJsonsAuto for tags: out as ProcessJsons with want_tags = true.  text != nullptr: the caller wants
    // the result document ('[' D0 ',' D1 ... ']', tags_json.hpp); when the device route answers and writes it (gft_tagdoc.hip),
    // text->written is set, the entries never cross the link and `out` stays empty
    int TagJsonsSchema(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, std::vector<DocResult>& out, Error& err,
                       ResultText* text = nullptr);
    int TagJsonsAuto(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const std::vector<std::string>& includePaths,
                     const std::vector<std::string>& excludePaths, std::vector<DocResult>& out, Error& err, ResultText* text = nullptr);
    // ---- the tag result document as text (tags_json.hpp, gft_tagdoc.hip): depends on the finder's expressions and on the schema.
    // device pointers except total: a leaf bitmap [n_leaves][ceil(E / 32)] with the record arrays of TagRecordsDevice -> text and
    // out_off [n_records + 1] under the cap protocol; d_hole_len nullable.  GFT_E_UNSUPPORTED: tables the format cannot hold, and
    // what the contract refuses of a batch (a field twice, a record beyond GFT_TAGS_JSON_MAX_LEAVES, a document of 4 GiB)
    int TagsJsonDevice(const uint32_t* d_hit_bitmap, const uint32_t* d_leaf_field, const uint64_t* d_rec_off, uint64_t n_records, uint64_t n_leaves,
                       const uint64_t* d_hole_len, uint8_t* d_out, uint64_t cap, uint64_t* d_out_off, uint64_t* total, Error& err);
    // tags_json_host over the finder's current expressions and the schema: no device
    int DebugTagsJson(const uint32_t* hit_bitmap, uint32_t n_exprs, const uint32_t* leaf_field, const uint64_t* rec_off, uint64_t n_records,
                      uint64_t n_leaves, const uint64_t* hole_len, uint8_t* out, uint64_t cap, uint64_t* out_off, uint64_t* total, Error& err);
    // tag_entries_host, and the three launches, over a caller-supplied leaf bitmap (host / device pointers)
    int DebugTagEntries(const uint32_t* hit_bitmap, uint32_t n_exprs, const uint32_t* leaf_field, const uint64_t* rec_off, uint64_t n_records,
                        uint64_t n_leaves, const TagEntries& out, Error& err);
    int DebugTagEntriesDevice(const uint32_t* d_hit_bitmap, uint32_t n_exprs, const uint32_t* d_leaf_field, const uint64_t* d_rec_off,
                              uint64_t n_records, uint64_t n_leaves, const TagEntries& d_out, Error& err);

    // the compiled device words interpreted on the host over a caller-supplied leaf bitmap: no device
    int DebugEvalRules(const uint32_t* hit_bitmap, uint32_t n_exprs, const uint32_t* leaf_field, const uint64_t* rec_off, uint64_t n_records,
                       uint64_t n_leaves, uint32_t* rule_bitmap, Error& err);

    // the two kernels over a caller-supplied leaf bitmap on the device (the device half of the proof: what the kernels make of
    // rows the finder did not write, bits at and above n_exprs included)
    int DebugEvalRulesDevice(const uint32_t* d_hit_bitmap, uint32_t n_exprs, const uint32_t* d_leaf_field, const uint64_t* d_rec_off,
                             uint64_t n_records, uint64_t n_leaves, uint32_t* d_rule_bitmap, Error& err);

    const RuleMap& rules() const { return rules_; }
    const std::set<std::string>& fields() const { return fields_; }
    const std::set<std::string>& tags() const { return tags_; }
    // leaves and bytes of the last TagJsons call (measurement)
    uint64_t last_leaves = 0, last_bytes = 0;

private:
    Finder* findthem_;
    RuleMap rules_;
    std::set<std::string> fields_, tags_;

    uint64_t rules_version_ = 0;           // counts AddRule calls that changed rules_
    std::vector<RuleExpr> rule_exprs_;
    uint64_t rule_exprs_version_ = ~0ull;

    // ---- the rules' fragment table (rules_json.hpp), rebuilt when rules_version_ changes; rec_ and auto_ share it
    static bool env_device_result();       // GFT_DEVICE_RESULT=0: the result documents are serialised on the host (read at creation)
    bool device_result_;
    std::shared_ptr<RuleFragments> frags_; // null with frags_version_ current: refused, `frags_why_` says why
    uint64_t frags_version_ = ~0ull, frags_serial_ = 0;
    Error frags_why_;
    const RuleFragments* fragments();      // the table for the current rules, or null
    int result_ready(gft_engine* e, Error& err);   // ... installed on e, unless it is the one the engine holds (fragments() != null)

    // ---- the tag document's tables (tags_json.hpp): the slot part is the group's, rebuilt when the finder has more expressions;
    // the field part is a Records' (made once: a Records' schema and lists do not change)
    std::shared_ptr<TagSlots> tslots_;     // null with tslots_n_exprs_ current: refused, `tslots_why_` says why
    size_t tslots_n_exprs_ = ~(size_t)0;
    uint64_t tslots_serial_ = 0;
    Error tslots_why_;
    const TagSlots* tag_slots();
    struct Records;
    const TagFields* tag_fields(Records& r);
    // both tables for r, or GFT_E_UNSUPPORTED with the reason; e != nullptr: installed on e unless they are what the engine holds
    int tagdoc_ready(gft_engine* e, Records& r, Error& err);
    // under the caller's RulesLock: the staged JSON batch's tag document written on the device into `text`, the documents the
    // device did not decide (or that are wider than GFT_TAGS_JSON_MAX_LEAVES) serialised on the host and copied into their holes
    int json_tag_text(gft_engine* e, Records& r, const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const uint8_t* d_blob,
                      const uint64_t* d_doc_off, uint8_t* d_status, std::string& text, Error& err);

    // ---- a schema with what was compiled from it (group_records.hpp).  Every helper names the Records it works on: rec_ is
    // SetSchema's, auto_ the one ProcessJsonsAuto keeps between its calls, and neither route touches the other's.
    std::shared_ptr<Records> rec_, auto_;
    Records* schema_records(const char* what, Error& err);   // rec_, or "<what>: no schema set (gft_group_set_schema)"
    // the one way to a Records: the rule set (compile_set), then the trie into json / json_rc / json_err.  Returns the rule
    // compiler's status; what a refused trie means is the caller's to say
    int make_records(const std::vector<std::string>& paths, const std::vector<std::string>& includePaths,
                     const std::vector<std::string>& excludePaths, Records& out, Error& err);
    int compile_set(Records& r, Error& err);               // r.set from r's schema and lists, stamped; untouched on a refusal
    int compile(Records& r, Error& err);                   // ... when rules or finder expressions were added since
    int install(gft_engine* e, Records& r, Error& err);    // r.set on the engine, unless it is the one the engine holds
    int json_ready(gft_engine* e, Records& r, Error& err); // r's trie: refused, or installed on e (e == nullptr: checked only)
    // What a device call over records is to produce (group_records.hpp): rule rows, or tag entries
    struct RecordsOut;
    int records_device(Records& r, const uint8_t* d_text, const uint64_t* d_leaf_off, const uint32_t* d_leaf_field, const uint64_t* d_rec_off,
                       uint64_t n_records, uint64_t n_leaves, const RecordsOut& out, Error& err);    // ProcessRecordsDevice, TagRecordsDevice
    int jsons_device(Records& r, const uint8_t* d_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint8_t* d_status, const RecordsOut& out,
                     Error& err);                                                                    // ProcessJsonsDevice, TagJsonsDevice
    // ---- a JSON batch from host memory, for ProcessJsonsSchema / ProcessJsonsAuto (want_tags == false: rule rows) and
    // TagJsonsSchema / TagJsonsAuto (want_tags == true: tag entries): a finder that does not qualify sends it through ProcessJsons
    // (with the lists given); else the batch is uploaded (rule rows: with rows of row_words words) and, under the engine's lock,
    // `choose` names the Records that answer it -- null with rc == 0: ProcessJsons after all.
    // lines != nullptr: the batch is a blob of lines->len bytes of JSON Lines -- doc_off and n_docs are not read; the blob is cut
    // where it is staged (or by split_lines_host on the host route) and lines->off receives the offsets the routes go on with.
    struct JsonLines { uint64_t len = 0; std::vector<uint64_t> off; };
    using ChooseRecords = std::function<std::shared_ptr<Records>(gft_engine* e, const uint8_t* d_blob, const uint64_t* d_doc_off, uint64_t n_docs, int& rc)>;
    int json_batch(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const std::vector<std::string>& includePaths,
                   const std::vector<std::string>& excludePaths, bool want_tags, uint64_t row_words, const ChooseRecords& choose,
                   std::vector<DocResult>& out, Error& err, ResultText* text = nullptr, JsonLines* lines = nullptr);
    // what came down from the device for a staged batch: the status bytes, and the rule rows or the tag entries
    struct JsonStaged;
    // under the caller's RulesLock: jsons_device over the staged batch, status and rows / entries down ...
    // (fetch_rows == false: the rule rows stay in d_rows)
    int json_staged(gft_engine* e, Records& r, const uint8_t* d_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint8_t* d_status,
                    uint32_t* d_rows, bool want_tags, JsonStaged& s, Error& err, bool fetch_rows = true);
    // the documents the device did not decide (status != 0), through ProcessJsons as one sub-batch: res[k] is document host_docs[k]'s
    int json_host_docs(const Records& r, const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const std::vector<uint8_t>& status,
                       bool want_tags, std::vector<uint64_t>& host_docs, std::vector<DocResult>& res, Error& err);
    // under the caller's RulesLock, behind json_staged without the rows: the undecided documents serialised on the host and left as
    // holes, the text written on the device from d_rows, brought down into `text` and the holes copied in
    int json_text(gft_engine* e, const Records& r, const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const uint32_t* d_rows,
                  const JsonStaged& s, std::string& text, Error& err);
    // ... and behind it: the documents the device did not decide through ProcessJsons as one sub-batch, the others from their rows
    // or entries, a document per task
    int json_results(const Records& r, const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const JsonStaged& s, bool want_tags,
                     std::vector<DocResult>& out, Error& err);
    int jsons_schema(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, bool want_tags, std::vector<DocResult>& out, Error& err,
                     ResultText* text = nullptr, JsonLines* lines = nullptr);
    int jsons_auto(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, const std::vector<std::string>& includePaths,
                   const std::vector<std::string>& excludePaths, bool want_tags, std::vector<DocResult>& out, Error& err,
                   ResultText* text = nullptr, JsonLines* lines = nullptr);
};

}  // namespace gft
