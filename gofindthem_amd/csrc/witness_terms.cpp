// witness_terms.cpp -- the witness table of gft_hit_spans_device (witness_terms.hpp).
#include "witness_terms.hpp"

#include <algorithm>
#include <utility>

#include "../../include/gft.h"

namespace gft {

int compile_witness_terms(const uint32_t* prog_words, const uint64_t* prog_off, uint32_t n_exprs, uint32_t n_terms, uint32_t n_slots,
                          WitnessTable& out) {
    if (n_exprs && (!prog_words || !prog_off)) return GFT_E_INVALID;
    std::vector<std::pair<uint32_t, uint32_t>> pairs;      // (term, expression), expression-major
    std::vector<std::vector<uint32_t>> stack;
    for (uint32_t i = 0; i < n_exprs; i++) {
        if (prog_off[i + 1] < prog_off[i]) return GFT_E_INVALID;
        stack.clear();
        for (uint64_t k = prog_off[i]; k < prog_off[i + 1]; k++) {
            const uint32_t w = prog_words[k], op = w >> 28;
            if (op == GFT_OP_UNIT) {
                const uint32_t slot = w & GFT_SLOT_MASK;
                if (slot >= n_slots) return GFT_E_INVALID;
                stack.emplace_back();
                if (slot < n_terms) stack.back().push_back(slot);
            } else if (op == GFT_OP_AND || op == GFT_OP_OR) {
                if (stack.size() < 2) return GFT_E_INVALID;
                // (the shorter set goes into the longer: a chain of any length costs its units once)
                std::vector<uint32_t>& a = stack[stack.size() - 2];
                std::vector<uint32_t>& b = stack.back();
                if (a.size() < b.size()) a.swap(b);
                a.insert(a.end(), b.begin(), b.end());
                stack.pop_back();
            } else if (op == GFT_OP_NOT) {
                if (stack.empty()) return GFT_E_INVALID;
                stack.back().clear();
            } else if (op == GFT_OP_INORD) {
                if (stack.empty()) return GFT_E_INVALID;
            } else {
                return GFT_E_INVALID;
            }
        }
        if (stack.size() != 1) return GFT_E_INVALID;
        std::vector<uint32_t>& p = stack.back();
        std::sort(p.begin(), p.end());
        p.erase(std::unique(p.begin(), p.end()), p.end());
        for (uint32_t t : p) pairs.emplace_back(t, i);
    }
    WitnessTable tab;
    tab.off.assign((size_t)n_terms + 1, 0);
    for (const auto& pr : pairs) tab.off[pr.first + 1]++;
    for (uint32_t t = 0; t < n_terms; t++) tab.off[t + 1] += tab.off[t];
    tab.expr.assign(pairs.size(), 0);
    std::vector<uint64_t> at(tab.off.begin(), tab.off.end() - 1);
    for (const auto& pr : pairs) tab.expr[at[pr.first]++] = pr.second;     // (expression-major input: ascending per term)
    out = std::move(tab);
    return GFT_OK;
}

}  // namespace gft
