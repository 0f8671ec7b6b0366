// rule_words.hpp -- limits and word format of the record rule programs, shared by the compiler (rule_set.cpp) and the
// kernels (gft_rules.hip)
#pragma once
#include <stdint.h>

namespace gft {

constexpr uint32_t kRuleMaxUnits = 8192;         // distinct (tag, prefix) pairs: a 64-bit word each in LDS
constexpr uint32_t kRuleMaxDepth = 32;           // operand-stack depth of one program
constexpr uint32_t kRuleMaxFields = 65535;       // schema entries
constexpr uint32_t kRuleNoTag = 0xFFFFFFFFu;     // a UNIT whose tag the finder does not know: never true
constexpr uint32_t kRuleBlock = 256;             // threads of k_record_rules: 64 records per workgroup, 256 rules per trip
// program word = op << 28 | operand
enum RuleOp : uint32_t { kRopUnit = 1, kRopAnd = 2, kRopOr = 3, kRopNot = 4 };

}  // namespace gft
