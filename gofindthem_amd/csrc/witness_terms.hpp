// witness_terms.hpp -- which keywords explain a true expression: public postfix programs (include/gft.h) -> the witness table of
// gft_hit_spans_device.  P(i), the witness terms of expression i, are the dictionary slots (slot < n_terms) of its GFT_OP_UNIT
// words that lie outside the operand of every GFT_OP_NOT: one walk over the words with a stack of unit sets, a NOT empties the
// top set (and nothing restores it: a unit under two NOTs is no witness either), AND / OR join the two top sets, INORD changes
// nothing.  Extra slots (>= n_terms) are never witnesses; a slot that occurs twice is listed once.  The table is the inverse,
// term -> expressions: wit_expr[wit_off[t] .. wit_off[t + 1]) ascending.  Host arithmetic only: no device, no handle.
#pragma once
#include <cstdint>
#include <vector>

namespace gft {

struct WitnessTable {
    std::vector<uint64_t> off;     // [n_terms + 1]
    std::vector<uint32_t> expr;    // [off[n_terms]]
};

// GFT_OK, or GFT_E_INVALID for a program that is no postfix expression (an operator without its operands, more than one value
// left, an unknown opcode, a slot >= n_slots, offsets that descend) -- `out` is then untouched.
int compile_witness_terms(const uint32_t* prog_words, const uint64_t* prog_off, uint32_t n_exprs, uint32_t n_terms, uint32_t n_slots,
                          WitnessTable& out);

}  // namespace gft
