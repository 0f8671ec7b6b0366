// rules_json.hpp -- the result document of a batch's rule rows as text: the fragment table the device copies from, and the
// contract of gft_result.hip stated in plain loops.  Pure: no device, no handle.  It is gft_debug_rules_json and what the
// device kernels are compared with.
//
//   text = '[' D0 ',' D1 ',' ... ']',   Dd = {"rules":{ members }}
//   a member per rule with a set bit, in bit order: json_str(name) ":[" the rule's true expressions, each json_str(expr),
//   joined by ',' then ']'; members joined by ','.  A row without bits: {"rules":{}}.
//
// That is byte for byte what gft_group_process_jsons' result document is for DocResults with those rules: the bits of a row are
// ascending rule name, then AddRule order inside a name -- the iteration order of the std::map and of its vectors.
#pragma once
#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "group_host.hpp"

namespace gft {

constexpr uint32_t kRuleDocFixed = 12;     // {"rules":{ and }}: every document is at least this long, so 0 can mean "no hole"
constexpr uint32_t kRuleFragSlack = 16;    // readable bytes behind the blob

// Per rule expression i (bit i of a rule row): where its rule begins, its rule's name fragment json_str(name) + ":[" (the same
// for every expression of a rule) and its own fragment json_str(expr), as offset and length into one blob of escaped bytes.
struct RuleFragments {
    std::vector<uint32_t> rule_first, name_off, name_len, expr_off, expr_len;   // [R]
    std::vector<uint8_t> blob;                                                   // the fragments, then kRuleFragSlack zero bytes
    uint32_t n_exprs() const { return (uint32_t)rule_first.size(); }
};

// false: a table the format cannot hold -- the blob, with every document's frame, would not fit 32-bit lengths -- and `why`
// says so.  Never the caller's error: such a group serialises on the host.
bool make_rule_fragments(const std::vector<GroupFinder::RuleExpr>& exprs, RuleFragments& out, std::string& why);

// rule rows [n_docs][ceil(R / 32)] -> the text and out_off [n_docs + 1]: out_off[0] = 1, out_off[d + 1] = out_off[d] + len(d) + 1,
// the separator behind document d (',' or the closing ']') at out_off[d + 1] - 1.  hole_len (nullable) [n_docs]: a value != 0
// reserves exactly that many bytes for document d, none of them is written and its row is not read.  A byte at a position >= cap
// is not stored; *total (nullable) = the text's size (2 for n_docs == 0: "[]").  out == nullptr with cap == 0 counts only.
// false: a hole of 4 GiB or more (nothing is complete then).
bool rules_json_host(const RuleFragments& fr, const uint32_t* rule_bitmap, uint64_t n_docs, const uint64_t* hole_len, uint8_t* out, uint64_t cap,
                     uint64_t* out_off, uint64_t* total);

// One document of the host serialisation: {"error": json_str(err)} or {"rules":{..}} -- what a hole's text is
void rule_doc_text(const std::string& err, const std::map<std::string, std::vector<std::string>>& rules, std::string& o);

}  // namespace gft
