// gft_words.hpp -- whole-word matching (gft_words.hip): the launchers, the class table, and the same walk on the host
// (words_host.cpp).
#pragma once
#include <stdint.h>

#include "../../include/gft.h"
#include "gft_select.hpp"
#include "gft_words_piece.hpp"

namespace gft {

// entries and documents of one filter call: the place pass's grid stays below 2^31
constexpr uint64_t kWordsMax = 1ull << 38;

// the class table of unicode_word.inc in host memory, and its size in rows of 256 bits
const WordTable& word_table_host();
uint32_t word_table_rows();

// gft_filter_word_matches_device's contract on host pointers: the check pass, then mark, prefix sum and place, entry tile by entry
// tile through gft_words_piece.hpp.  Returns a gft_status; a refusal writes nothing.
int filter_word_matches_host(const uint8_t* text, const uint64_t* doc_off, uint64_t n_docs, const uint64_t* off, const uint32_t* pos,
                             const uint32_t* len, const uint32_t* term, const uint32_t* term_len, uint32_t n_terms, uint32_t flags,
                             uint64_t* out_off, uint32_t* out_pos, uint32_t* out_len, uint32_t* out_term, uint64_t cap, uint64_t* total);

// an output of the filter (out_off [n_docs + 1], three arrays of cap words) overlaps one of the n_in input ranges, or another
inline bool words_outputs_overlap(const uint64_t* out_off, uint64_t n_docs, const uint32_t* o0, const uint32_t* o1, const uint32_t* o2, uint64_t cap,
                                  const ByteRange* ins, size_t n_in) {
    const ByteRange outs[] = {{out_off, out_off ? (n_docs + 1) * 8 : 0}, {o0, cap * 4}, {o1, cap * 4}, {o2, cap * 4}};
    return outputs_overlap(outs, 4, ins, n_in);
}

}  // namespace gft

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

struct gft_engine;

namespace gft {

// the class table on the device (e->d_words.tab_row / tab_bits): uploaded by the first call of a handle that needs it, under the
// caller's lock and DeviceGuard.  Returns a gft_status (gft_words_api.cpp)
int ensure_word_table(gft_engine* e);

// Work buffers: 16 bytes of flag words, 4 bytes of marks and 8 bytes of ranks an entry, the prefix sum's partials.
struct WordsParams {
    const uint8_t* text;
    const uint64_t* doc_off;       // [n_docs + 1]
    uint64_t n_docs;
    const uint64_t* off;           // [n_docs + 1]   the list's CSR; the entries are [e0, e0 + n)
    uint64_t e0, n;
    const uint32_t* pos;
    const uint32_t* len;           // NULL: the length is term_len[term[i]]
    const uint32_t* term;          // NULL, or carried through
    const uint32_t* term_len;      // [n_terms]
    uint32_t n_terms, pos_end;
    WordTable table;               // the device copy
    uint32_t* ctl;                 // [kWordsCtlWords]  check
    uint32_t* keep;                // [n]               mark
    const uint64_t* rank;          // [n + 1]           exclusive prefix sum of keep
    uint64_t* out_off;             // [n_docs + 1] or NULL
    uint32_t* out_pos;             // [cap] or NULL
    uint32_t* out_len;
    uint32_t* out_term;
    uint64_t cap;
};

hipError_t launch_words_check(const WordsParams& P, unsigned n_cus, hipStream_t st);
hipError_t launch_words_mark(const WordsParams& P, unsigned n_cus, hipStream_t st);
hipError_t launch_words_place(const WordsParams& P, hipStream_t st);

}  // namespace gft
#endif
