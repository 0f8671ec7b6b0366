// rule_set.hpp -- the group finder's rule compiler for records (a batch of (field, string) leaves instead of JSON documents):
// parsed rules + the finder's tags + a schema of field paths + include / exclude paths -> everything gft_rules.hip reads.
// A rule expression is a Boolean algebra over "tag T was matched in a valid field whose path starts with P"
// (group/dsl/expression.go:68-125): per distinct prefix a bit mask over the schema, per distinct (tag, prefix) a UNIT, per
// expression a postfix program over the UNITs.  Host arithmetic only: no device, no handle -- rules_install (gft_rules.hpp) uploads what
// comes out, eval_rules_host interprets the same words on the CPU.
#pragma once
#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "../../include/gft.h"
#include "group_dsl.hpp"
#include "rule_words.hpp"

namespace gft {

struct RuleSet {
    uint32_t n_fields = 0, n_tags = 0, n_exprs = 0, n_rules = 0;
    uint32_t field_words = 0;              // ceil(n_fields / 32): words of one mask
    std::vector<uint32_t> valid;           // [field_words] IsValidFieldPath per schema entry (exclude wins over include)
    std::vector<uint32_t> masks;           // [n_masks][field_words] bit f: valid[f] && path[f] starts with the prefix
    std::vector<std::string> prefixes;     // [n_masks] the prefix of every mask, in order of first use
    std::vector<uint32_t> units;           // [n_units][2] = tag id (kRuleNoTag: constant false), mask id
    std::vector<uint32_t> prog;            // postfix programs, one per rule expression in the order of GroupFinder::rules()
    std::vector<uint32_t> prog_off;        // [n_rules + 1]
    std::vector<uint32_t> depth;           // [n_rules] operand-stack depth of every program
    std::vector<uint32_t> expr_tag;        // [n_exprs] tag id of every finder expression
    uint32_t max_depth = 0;
    uint32_t n_masks() const { return field_words ? (uint32_t)(masks.size() / field_words) : (uint32_t)prefixes.size(); }
    uint32_t n_units() const { return (uint32_t)(units.size() / 2); }
};

// Compiles a whole set.  GFT_OK, or the status of the first refusal with its text in `err` -- `out` is then untouched.
// rules: GroupFinder::rules() (ascending rule name, AddRule order inside a name); tags / expr_tag: Finder::tags() /
// Finder::tag_ids(); schema: unique field paths as getRulesInfo builds them.
int compile_rules(const RuleMap& rules, const std::vector<std::string>& tags,
                  const std::vector<uint32_t>& expr_tag, const std::vector<std::string>& schema,
                  const std::vector<std::string>& includePaths, const std::vector<std::string>& excludePaths, RuleSet& out, std::string& err);

// The two kernels of gft_rules.hip on the host, over the compiled words: hit rows [n_leaves][ceil(n_exprs / 32)] -> tag rows
// -> UNIT answers -> rule_bitmap [n_records][ceil(n_rules / 32)].  The batch must have been validated (validate_records).
void eval_rules_host(const RuleSet& rs, const uint32_t* hit_bitmap, const uint32_t* leaf_field, const uint64_t* rec_off, uint64_t n_records,
                     uint32_t* rule_bitmap);
// "" or what is wrong with a batch in host memory: a field index outside the schema, offsets that descend or do not end at n_leaves
std::string validate_records(uint32_t n_fields, const uint32_t* leaf_field, const uint64_t* rec_off, uint64_t n_records, uint64_t n_leaves);

}  // namespace gft
