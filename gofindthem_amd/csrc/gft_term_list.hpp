// gft_term_list.hpp -- the (off, term) list of a resident batch, for the batch calls that count it or rank by it
// (gft_batch_term_stats_device, gft_batch_top_docs_device and their whole-word twins), and the head that the calls which take such
// a list share (gft_term_stats_device, gft_score_docs_device).  All of it runs behind the caller's lock (gft_term_list.cpp).
#pragma once
#include "gft_engine.hpp"
#include "gft_stats.hpp"

namespace gft::api {

// One batch call's question.  who: the entry point that was called (every refusal of the front end's own names it); words: the
// whole-word sources; flags / known_flags: the caller's own flag word and the bits it knows; top: a top call, whose k and top
// arrays are tested in front of the scan; room: what a failed allocation of the kept list says
struct BatchList {
    const char* who; bool words;
    const uint8_t* d_text; const uint64_t* d_doc_off; uint64_t n_docs;
    uint32_t scan_flags; const uint32_t* d_hit_bitmap; const uint32_t* want;
    uint32_t flags, known_flags;
    bool top; uint32_t k; const uint64_t* d_top_idx; const uint64_t* d_top_score;
    RoomTexts room;
};
// the list on the device: off NULL for a batch without documents.  Without a bitmap it is the scan's own list and holds until the
// handle's next scan; with one it is e->d_kept and holds until the next batch call
struct TermList { const uint64_t* off; const uint32_t* term; };

// Which list does this batch give?  Refuses, in this order: null arguments, flag bits (the caller's, then scan_flags), k and the
// top arrays, handles over several devices, a handle without a device, an n_docs beyond the source's limit -- and only then
// allocates.  The source is gft_scan_device / gft_scan_words_device without a bitmap, and gft_hit_spans_device /
// gft_hit_spans_words_device with one (the matches that witness a hit of a wanted expression; counted, then filled into e->d_kept).
// The call is a scan: the batch's verdict is published.  With GFT_FOLD_ASCII, documents and a batch that is not fold-safe,
// *nonascii = 1, GFT_OK and no list (the caller returns; nothing of its own has been written); with nonascii NULL the call goes on.
int batch_term_list(gft_engine* e, const BatchList& A, TermList& out, int* nonascii);

// The head of a call that takes a list (d_off [n_docs + 1], d_term), behind the caller's tests of the handle and of n_docs, under
// its DeviceGuard: the list's two ends read back, and what they alone refuse -- offsets that descend, a size beyond the address
// space, entries without d_term or without terms.  The entries are [e0, e0 + n).  Waits for the stream.
struct ListEnds { uint64_t e0, n; };
int list_head(gft_engine* e, const char* who, const uint64_t* d_off, const uint32_t* d_term, uint64_t n_docs, uint32_t n_terms, ListEnds& L);
// the check pass over that list, its two flag words into ctl (zeroed by the caller); stage: "stats" or "score", as the profile
// category and the launch's failure name it
int list_check_launch(gft_engine* e, const char* stage, const uint64_t* d_off, const uint32_t* d_term, uint64_t n_docs, const ListEnds& L,
                      uint32_t n_terms, uint64_t* ctl);
// what the check pass found (the control block read back): offsets that descend inside the list, a term id that is no index of
// `indexed` ("the counters", "the weights")
int list_check_verdict(gft_engine* e, const char* who, const uint64_t* h_ctl, const char* indexed);

}  // namespace gft::api
