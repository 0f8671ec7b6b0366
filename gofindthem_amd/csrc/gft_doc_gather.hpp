// gft_doc_gather.hpp -- the front end the document-gather calls share (select, context, route), and the select's copy pass over
// compact arrays, which the excerpts take too.  A call goes: its own argument refusals (their order differs from call to call),
// empty, its own work buffers, mark, its own passes, read, its own overlap list, its own outputs and compact arrays, its own place pass, copy.
// It owns the SyncOnExit: the host memory the asynchronous copies read is the entry point's.
#pragma once
#include "gft_engine.hpp"
#include "gft_select.hpp"

namespace gft::api {

struct DocGather {
    const char* who;               // the entry point the refusals name
    const char* word;              // the call's word in what fail_hip names and in its stages: "<word> totals", "<word>_mark", ...
    RoomTexts room;
};

// the m entries c_off [m + 1] / c_src [m] of `text`, `total` bytes of them, into out[0, cap_bytes) under the gft_profile_read
// name `stage` (no byte to write: no launch, no stage).  what: what fail_hip names
int select_copy_run(gft_engine* e, const uint8_t* text, const uint64_t* c_off, const uint64_t* c_src, uint64_t m, uint64_t total, uint8_t* out,
                    uint64_t cap_bytes, const char* stage, const char* what);

// no documents: out_off[0] = 0 (and group_off[0], for the call that has groups), and the synchronisation
int doc_gather_empty(gft_engine* e, const DocGather& G, uint64_t* d_out_off, uint64_t* d_group_off = nullptr);
// The select's mark run under "<word>_mark": M's inputs and mark outputs filled in from the call's arguments and buffers (which
// have their room), h_want uploaded, ctl_words words of the control block cleared, k_select_mark launched.
int doc_gather_select_mark(gft_engine* e, const DocGather& G, SelectParams& M, const uint8_t* d_text, const uint64_t* d_doc_off, uint64_t n_docs,
                           const uint32_t* d_bitmap, uint32_t n_cols, uint32_t mode, const uint8_t* d_also, const uint32_t* h_want, DevBuf& want,
                           DevBuf& len, DevBuf& sel, DevBuf& ctl, uint32_t ctl_words);
// n_words words of the control block into h_ctl (one synchronisation); refuses on the word kSelCtlFlag.  The text's range for the
// call's own overlap list is then in the words kSelCtlLo and kSelCtlHi, and doc_gather_overlap is what that list's refusal says.
int doc_gather_read(gft_engine* e, const DocGather& G, const uint64_t* d_ctl, uint64_t* h_ctl, uint64_t n_words);
int doc_gather_overlap(const gft_engine* e, const DocGather& G);
// the tail behind the call's place pass: the copy under "<word>_copy" and the final synchronisation
int doc_gather_copy(gft_engine* e, const DocGather& G, const uint8_t* text, const uint64_t* c_off, const uint64_t* c_src, uint64_t m, uint64_t total,
                    uint8_t* out, uint64_t cap_bytes);

}  // namespace gft::api
