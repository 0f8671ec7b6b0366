// C++ mirror of the reference's finder package API (finder/finder.go, finder/substringEngine.go,
// finder/regexEngine.go) on top of the GPU engine.  Same names, argument meaning and error behaviour; the Go
// `error` value is a std::string here ("" == nil).
#pragma once
#include <cstdint>
#include <memory>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/gft.h"
#include "dsl_compile.hpp"

namespace gft {

using Error = std::string;

// finder.Match (finder/finder.go:11-14)
struct Match {
    int64_t Position;
    std::string Term;
};

// finder.ExpressionResult (finder/finder.go:25-29; field names sic)
struct ExpressionResult {
    int ExpresionIndex;
    std::string ExpresionStr;
    std::string Tag;
};

// finder.SubstringEngine (finder/substringEngine.go:11-18)
class SubstringEngine {
public:
    virtual ~SubstringEngine() {}
    virtual Error BuildEngine(const std::vector<std::string>& keywords, bool caseSensitive) = 0;
    virtual Error FindSubstrings(const std::string& text, std::vector<Match>& matches) = 0;
};

// finder.RegexEngine (finder/regexEngine.go:8-15)
class RegexEngine {
public:
    virtual ~RegexEngine() {}
    virtual Error BuildEngine(const std::vector<std::string>& regexes, bool caseSensitive) = 0;
    virtual Error FindRegexes(const std::string& text, std::vector<Match>& matches) = 0;
};

// finder.EmptyEngine / finder.EmptyRgxEngine (substringEngine.go:121-133, regexEngine.go:49-60)
class EmptyEngine : public SubstringEngine {
public:
    Error BuildEngine(const std::vector<std::string>&, bool) override { return ""; }
    Error FindSubstrings(const std::string&, std::vector<Match>&) override { return ""; }
};
class EmptyRgxEngine : public RegexEngine {
public:
    Error BuildEngine(const std::vector<std::string>&, bool) override { return ""; }
    Error FindRegexes(const std::string&, std::vector<Match>&) override { return ""; }
};

// The drop-in for finder.CloudflareForkEngine: same two methods, backed by libgft's HIP kernels.
class GpuEngine : public SubstringEngine {
public:
    explicit GpuEngine(int device = -1);
    // one engine over several devices (gft_engine_create_multi): batches are sharded across them by the library
    GpuEngine(const int* devices, int n_devices);
    ~GpuEngine() override;
    Error BuildEngine(const std::vector<std::string>& keywords, bool caseSensitive) override;
    Error FindSubstrings(const std::string& text, std::vector<Match>& matches) override;
    gft_engine* handle() const { return h_; }
    const Error& create_error() const { return create_err_; }
    uint64_t builds() const { return builds_; }
private:
    gft_engine* h_ = nullptr;
    Error create_err_;
    uint64_t builds_ = 0;
};

// engines supplied through the C ABI as callbacks (foreign implementations, test mocks)
class CallbackSubEngine : public SubstringEngine {
public:
    CallbackSubEngine(gft_engine_build_fn b, gft_engine_find_fn f, void* u) : b_(b), f_(f), u_(u) {}
    Error BuildEngine(const std::vector<std::string>& keywords, bool caseSensitive) override;
    Error FindSubstrings(const std::string& text, std::vector<Match>& matches) override;
private:
    gft_engine_build_fn b_; gft_engine_find_fn f_; void* u_;
};
class CallbackRgxEngine : public RegexEngine {
public:
    CallbackRgxEngine(gft_engine_build_fn b, gft_engine_find_fn f, void* u) : b_(b), f_(f), u_(u) {}
    Error BuildEngine(const std::vector<std::string>& regexes, bool caseSensitive) override;
    Error FindRegexes(const std::string& text, std::vector<Match>& matches) override;
private:
    gft_engine_build_fn b_; gft_engine_find_fn f_; void* u_;
};

// finder.Finder (finder/finder.go:32-240)
class Finder {
public:
    // gpu: the engine whose kernels scan (when subEng is that same GpuEngine) and solve.
    Finder(SubstringEngine* subEng, RegexEngine* rgxEng, bool caseSensitive, GpuEngine* gpu);

    Error AddExpression(const std::string& expression) { return AddExpressionWithTag(expression, ""); }
    Error AddExpressions(const std::vector<std::string>& expressions);
    Error AddExpressionsWithTag(const std::vector<std::string>& expressions, const std::string& tag);
    Error AddExpressionWithTag(const std::string& expression, const std::string& tag);
    // returns the expressions that evaluated true, in registration order (never "nil": empty vector)
    Error ProcessText(const std::string& text, std::vector<ExpressionResult>& expRes);
    // batch extension: bitmap[d * words + (i >> 5)] bit (i & 31); words = ceil(n_expressions / 32)
    Error ProcessTexts(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, uint32_t* bitmap) {
        return process_texts(blob, doc_off, n_docs, bitmap, false);
    }
    // the batch form of ProcessText's result: document d's true expressions are expr_idx[row_off[d] .. row_off[d + 1]) in
    // registration order, tag_id[k] = tag id of expression expr_idx[k]; the arrays stay valid until the next call
    struct Sparse { const uint64_t* row_off = nullptr; const uint32_t* expr_idx = nullptr; const uint32_t* tag_id = nullptr; };
    Error ProcessTextsSparse(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, Sparse& out) {
        Error err = process_texts(blob, doc_off, n_docs, nullptr, true);
        if (err.empty()) out = sparse_;
        return err;
    }
    // gft_compact_device on the engine: a bitmap of ProcessDevice / ProcessDeviceBegin + End -> CSR on the device
    Error CompactDevice(const uint32_t* d_bitmap, uint64_t n_docs, uint64_t* d_row_off, uint32_t* d_expr_idx, uint32_t* d_tag_id,
                        uint64_t cap, uint64_t* total);
    // distinct tags in order of first registration ("" included), and the tag id of every expression
    const std::vector<std::string>& tags() const { return tags_; }
    const std::vector<uint32_t>& tag_ids() const { return tag_ids_; }
    Error ProcessDevice(const uint8_t* d_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint32_t* d_bitmap);
    // gft_split_lines_device on the finder's engine, for a blob that ProcessDevice is to take next: what ProcessDevice needs of the
    // finder, refused in its words
    Error SplitLinesDevice(const uint8_t* d_blob, uint64_t len, uint32_t mode, uint64_t* d_doc_off, uint64_t cap, uint64_t* n_docs);
    // gft_select_docs_device on the finder's engine over the rows ProcessDevice left (n_cols = the expressions): what ProcessDevice
    // needs of the finder, refused in its words
    Error SelectDocsDevice(const uint8_t* d_blob, const uint64_t* d_doc_off, uint64_t n_docs, const uint32_t* d_bitmap, const uint32_t* want,
                           uint32_t mode, const uint8_t* d_also, uint8_t* d_out, uint64_t cap_bytes, uint64_t* d_out_off, uint64_t* d_doc_idx,
                           uint64_t cap_docs, uint64_t* n_selected, uint64_t* total_bytes);
    // gft_context_docs_device on the finder's engine (n_cols = the expressions): what SelectDocsDevice asks, refused in its words
    Error ContextDocsDevice(const uint8_t* d_blob, const uint64_t* d_doc_off, uint64_t n_docs, const uint32_t* d_bitmap, const uint32_t* want,
                            uint32_t mode, const uint8_t* d_also, uint64_t before, uint64_t after, const uint8_t* d_fence, uint8_t* d_out,
                            uint64_t cap_bytes, uint64_t* d_out_off, uint64_t* d_doc_idx, uint8_t* d_kind, uint64_t cap_docs, uint64_t* d_group_off,
                            uint64_t cap_groups, uint64_t* n_kept, uint64_t* n_hits, uint64_t* n_groups, uint64_t* total_bytes);
    // gft_route_docs_device on the finder's engine (n_cols = the expressions): what SelectDocsDevice asks, refused in its words
    Error RouteDocsDevice(const uint8_t* d_blob, const uint64_t* d_doc_off, uint64_t n_docs, const uint32_t* d_bitmap, const uint32_t* masks,
                          uint32_t n_buckets, uint32_t mode, uint32_t flags, const uint8_t* d_also, uint8_t* d_out, uint64_t cap_bytes,
                          uint64_t* d_out_off, uint64_t* d_doc_idx, uint64_t cap_docs, uint64_t* bucket_doc, uint64_t* bucket_byte);
    // gft_hit_spans_device on the finder's engine under the finder's case rule: a batch that leaves ASCII is lowered on the device
    // and scanned again from there -- *lowered = 1: the spans index the lowered text.  What ProcessDevice asks, refused in its words.
    // source: the spans of a lowered batch are mapped back to the caller's bytes before the call returns (gft_map_spans_limit over
    // the entries below cap); cap != 0 then needs d_span_off and d_span_len
    Error HitSpansDevice(const uint8_t* d_blob, const uint64_t* d_doc_off, uint64_t n_docs, const uint32_t* d_bitmap, const uint64_t* d_row_idx,
                         const uint32_t* want, uint64_t* d_span_off, uint32_t* d_span_start, uint32_t* d_span_len, uint32_t* d_span_term, uint64_t cap,
                         uint64_t* total, int* lowered, bool source = false);
    // gft_excerpt_spans_device on the finder's engine behind HitSpansDevice: spans_lowered is what that call reported.  source (the
    // spans came from the source form of the call) or an unlowered batch: the excerpts are cut from the caller's batch; else from
    // the lowered text, which is lowered on the device again as the spans call lowered it -- *lowered = 1.  snap: the call is
    // gft_excerpt_spans_snap_device with `reach` (flags may then hold a snap bit)
    Error ExcerptsDevice(const uint8_t* d_blob, const uint64_t* d_doc_off, uint64_t n_docs, const uint64_t* d_span_off, const uint32_t* d_span_start,
                         const uint32_t* d_span_len, bool spans_lowered, bool source, uint32_t before, uint32_t after, uint32_t flags, uint8_t* d_out,
                         uint64_t cap_bytes, uint64_t* d_exc_off, uint64_t* d_exc_doc, uint32_t* d_exc_start, uint64_t* d_exc_span_off,
                         uint64_t cap_exc, uint32_t* d_span_rel, uint64_t* d_doc_exc_off, uint64_t* n_exc, uint64_t* total_bytes, int* lowered,
                         bool snap = false, uint32_t reach = 0);
    // gft_mark_spans_device on the finder's engine behind HitSpansDevice, under ExcerptsDevice's rule: source or an unlowered batch
    // marks the caller's batch; else the lowered text, lowered on the device again -- *lowered = 1
    Error MarkDevice(const uint8_t* d_blob, const uint64_t* d_doc_off, uint64_t n_docs, const uint64_t* d_span_off, const uint32_t* d_span_start,
                     const uint32_t* d_span_len, bool spans_lowered, bool source, const uint8_t* open, uint32_t open_len, const uint8_t* close,
                     uint32_t close_len, uint32_t flags, uint8_t* d_out, uint64_t cap_bytes, uint64_t* d_out_off, uint32_t* d_span_new,
                     uint64_t* d_doc_run_off, uint64_t* n_runs, uint64_t* total_bytes, int* lowered);
    // gft_replace_spans_device on the finder's engine behind HitSpansDevice, under MarkDevice's rule; term_rep: host, a replacement id
    // per term of the engine, NULL: id 0 for every term
    Error ReplaceDevice(const uint8_t* d_blob, const uint64_t* d_doc_off, uint64_t n_docs, const uint64_t* d_span_off, const uint32_t* d_span_start,
                        const uint32_t* d_span_len, bool spans_lowered, bool source, const uint32_t* d_span_term, const uint32_t* term_rep,
                        const uint8_t* rep_bytes, const uint64_t* rep_off, uint32_t n_reps, uint32_t flags, uint8_t* d_out, uint64_t cap_bytes,
                        uint64_t* d_out_off, uint64_t* d_doc_run_off, uint32_t* d_run_new, uint32_t* d_run_len, uint32_t* d_run_rep,
                        uint64_t cap_runs, uint64_t* n_runs, uint64_t* total_bytes, int* lowered);
    // gft_batch_term_stats_device on the finder's engine under the case rule of HitSpansDevice: a batch that leaves ASCII is lowered
    // on the device and counted from there -- *lowered = 1; an accumulating array sees every batch once
    Error TermStatsDevice(const uint8_t* d_blob, const uint64_t* d_doc_off, uint64_t n_docs, const uint32_t* d_bitmap, const uint32_t* want,
                          uint32_t flags, uint64_t doc_base, uint64_t* d_occ, uint64_t* d_docs, uint64_t* d_first, int* lowered);
    // gft_batch_top_docs_device (with the whole-word option its words twin) on the finder's engine under the same case rule: a batch
    // that leaves ASCII is lowered on the device and ranked from there -- *lowered = 1; document indices are those of the source
    Error TopDevice(const uint8_t* d_blob, const uint64_t* d_doc_off, uint64_t n_docs, const uint32_t* d_bitmap, const uint32_t* want,
                    const uint32_t* weights, uint32_t flags, uint32_t k, uint64_t doc_base, uint64_t* d_score, uint64_t* d_top_idx,
                    uint64_t* d_top_score, uint64_t* n_top, int* lowered);
    // pipelined: Begin enqueues (gft_process_device_begin), End completes the oldest batch begun, the ToLower repeat included
    Error ProcessDeviceBegin(const uint8_t* d_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint32_t* d_bitmap);
    Error ProcessDeviceEnd();
    Error ForceBuild();
    // whole-word matching (gft_words.hip): with the option on ProcessText / ProcessTexts / ProcessTextsSparse, ProcessDevice,
    // HitSpansDevice and TermStatsDevice answer from the occurrences that stand at word borders (gft_process_words*,
    // gft_hit_spans_words_device, gft_batch_term_stats_words_device); a foreign substring engine, regex terms or several devices
    // make every processing call fail with GFT_E_UNSUPPORTED, ProcessDeviceBegin always does
    void set_whole_words(bool on) { wholeWords_ = on; }
    bool whole_words() const { return wholeWords_; }
    const std::vector<std::string>& GetKeywords() const { return keywords_; }
    const std::vector<std::string>& GetRegexes() const { return regexes_; }

    struct ExprWrapper {
        std::string exprString;
        std::unique_ptr<dsl::Expression> expression;
        std::string tag;
    };
    const std::vector<ExprWrapper>& expressions() const { return expressions_; }
    int last_code() const { return last_code_; }
    // the engine behind ProcessDevice (nullptr: none), and whether ProcessDevice would take a batch: the GPU substring engine
    // and no regex terms
    gft_engine* device_engine() const { return gpu_ ? gpu_->handle() : nullptr; }
    bool device_resident_ok() const { return device_engine() && gpu_sub_ && regexes_.empty(); }
    uint64_t last_regex_docs = 0;        // documents the host regex engine saw in the last prefiltered ProcessTexts
    uint64_t lowered_on_device = 0, lowered_on_host = 0;   // batches of ProcessDevice / ProcessDeviceEnd repeated, by path
    bool force_host_lower_ = false;      // ProcessTexts is repeating a batch whose text the device cannot fold (finder_host.cpp)

    // test hooks (finder_test.go pokes the struct fields directly)
    void debug_add_literal(int which, const std::string& lit);
    bool updatedSubMachine = false, updatedRgxMachine = false;

private:
    struct Record { uint32_t slot, pos; };
    Error sync_device();
    Error fail_gft(int rc);
    void add_matches(const std::vector<Match>& ms, std::vector<Record>& out);
    Error collect(const std::string& lowered, bool run_sub, std::vector<Record>& out, bool run_rgx = true);
    Error process_texts_prefiltered(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, uint32_t* bitmap,
                                    uint32_t flags, bool need_host_text);
    // ProcessTexts (sparse == false: rows into bitmap) and ProcessTextsSparse (sparse == true: sparse_) are one function
    Error process_texts(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, uint32_t* bitmap, bool sparse);
    std::vector<std::string> tags_;
    std::unordered_map<std::string, uint32_t> tag_id_of_;
    std::vector<uint32_t> tag_ids_;      // per expression
    Sparse sparse_;                      // the last sparse result: the engine's buffers, or the three below (host route)
    std::vector<uint64_t> sp_row_off_;
    std::vector<uint32_t> sp_idx_, sp_tag_;

    // ---- regex prefilter.  With the GPU substring engine every regex that has required literals
    // (dsl::RegexRequiredLiterals) gets a hidden AND-of-literals program behind the user's expressions; the literals
    // join the device dictionary.  A batch is then solved once without regex hits, the host regex engine runs only on
    // the documents whose hidden programs fired, and the solver runs again (scan reused) if any of them matched.
    bool prefilter_active() const;
    const std::vector<std::string>& device_dictionary() const;   // keywords (+ hidden literals when the prefilter is active)
    mutable std::vector<std::string> dev_dict_;
    mutable bool dev_dict_ok_ = false, dev_dict_active_ = false;
    mutable size_t dev_dict_kw_ = 0, dev_dict_rx_ = 0;
    size_t total_programs() const { return expressions_.size() + (prefilter_active() ? regexes_.size() : 0); }
    std::vector<std::vector<std::string>> rgx_required_;    // per regex: literal runs every match contains

    std::vector<ExprWrapper> expressions_;
    std::vector<std::string> keywords_, regexes_;
    SubstringEngine* subEng_;
    RegexEngine* rgxEng_;
    bool caseSensitive_;
    bool wholeWords_ = false;
    Error words_refusal();               // "" or, with the option on, why this finder cannot match whole words (last_code_ set)
    Error resident_refusal();            // "" or why a resident batch cannot be taken: engine or regex terms, batches in flight (last_code_ set)
    GpuEngine* gpu_;
    bool gpu_sub_;                       // subEng_ is the GPU engine itself: scanning is fused into gft_process
    bool programs_dirty_ = true;
    bool empty_ready_ = false;           // we uploaded an empty dictionary ourselves (foreign engine / no keywords)
    uint64_t seen_builds_ = ~0ull;
    std::unordered_set<std::string> kw_set_, rgx_set_;
    std::unordered_map<std::string, uint32_t> slot_of_;
    Error solve_error_;                  // what Expression.Solve would return for every document, if anything
    int last_code_ = 0;
    struct Begun { const uint8_t* d_blob; const uint64_t* d_doc_off; uint64_t n_docs; uint32_t* d_bitmap; };
    Begun begun_[2] = {};                // batches of ProcessDeviceBegin that ProcessDeviceEnd has not completed yet
    unsigned first_begun_ = 0, n_begun_ = 0;
    bool device_tolower_;                // GFT_DEVICE_TOLOWER (read at creation; 0: a batch that leaves ASCII is lowered on the host)
    Error repeat_if_not_ascii(const uint8_t* d_blob, const uint64_t* d_doc_off, uint64_t n_docs, uint32_t* d_bitmap);
    // the two repeats of the resident-batch calls (finder_host.cpp): a call that scans, run again on the lowered batch if the batch
    // left ASCII; and a call that cuts from the text its spans index, handed the lowered batch when those are lowered spans
    template <class Run>
    Error scan_twice(const uint8_t* d_blob, const uint64_t* d_doc_off, uint64_t n_docs, const char* unsupported, int* lowered, Run run);
    Error cut_from_lowered(const char* what, bool spans_lowered, bool source, uint64_t n_docs, const uint8_t*& d_text, const uint64_t*& d_off,
                           int* lowered);
};

}  // namespace gft
