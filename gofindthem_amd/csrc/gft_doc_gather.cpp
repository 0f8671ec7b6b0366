// gft_doc_gather.cpp -- the front end the document-gather calls share (gft_doc_gather.hpp).
#include "gft_doc_gather.hpp"

namespace gft::api {

// what fail_hip names for a step of the call whose word is G.word
static std::string step(const DocGather& G, const char* what) { return std::string(G.word) + " " + what; }

int select_copy_run(gft_engine* e, const uint8_t* text, const uint64_t* c_off, const uint64_t* c_src, uint64_t m, uint64_t total, uint8_t* out,
                    uint64_t cap_bytes, const char* stage, const char* what) {
    SelectParams C{};                                               // (only what the copy reads is set)
    C.text = text; C.c_off = const_cast<uint64_t*>(c_off); C.c_src = const_cast<uint64_t*>(c_src); C.m = m; C.total = total; C.out = out;
    C.G = sel_geom(total, cap_bytes, out);
    if (C.G.end) {
        ProfScope ps(e, stage);
        HIP_TRY(launch_select_copy(C, e->stream), what);
    }
    return GFT_OK;
}

int doc_gather_empty(gft_engine* e, const DocGather& G, uint64_t* d_out_off, uint64_t* d_group_off) {
    const std::string what = step(G, "offsets");
    if (d_out_off) HIP_TRY(hipMemsetAsync(d_out_off, 0, 8, e->stream), what.c_str());
    if (d_group_off) HIP_TRY(hipMemsetAsync(d_group_off, 0, 8, e->stream), what.c_str());
    HIP_TRY(hipStreamSynchronize(e->stream), what.c_str());
    return GFT_OK;
}

int doc_gather_select_mark(gft_engine* e, const DocGather& G, SelectParams& M, const uint8_t* d_text, const uint64_t* d_doc_off, uint64_t n_docs,
                           const uint32_t* d_bitmap, uint32_t n_cols, uint32_t mode, const uint8_t* d_also, const uint32_t* h_want, DevBuf& want,
                           DevBuf& len, DevBuf& sel, DevBuf& ctl, uint32_t ctl_words) {
    M.text = d_text; M.doc_off = d_doc_off; M.n_docs = n_docs; M.bitmap = d_bitmap;
    M.W = (n_cols + 31) / 32; M.lg = bit_row_lg(M.W);
    M.mode = mode; M.want = want.as<uint32_t>(); M.also = d_also;
    M.len = len.as<uint32_t>(); M.sel = sel.as<uint32_t>(); M.ctl = ctl.as<uint64_t>();
    ProfScope ps(e, (std::string(G.word) + "_mark").c_str());
    if (M.W) HIP_TRY(hipMemcpyAsync(want.p, h_want, (size_t)M.W * 4, hipMemcpyHostToDevice, e->stream), step(G, "mask upload").c_str());
    HIP_TRY(hipMemsetAsync(M.ctl, 0, ctl_words * 8, e->stream), step(G, "mark").c_str());
    HIP_TRY(launch_select_mark(M, e->n_cus, e->stream), step(G, "mark kernel launch").c_str());
    return GFT_OK;
}

int doc_gather_read(gft_engine* e, const DocGather& G, const uint64_t* d_ctl, uint64_t* h_ctl, uint64_t n_words) {
    const std::string what = step(G, "totals");
    HIP_TRY(hipMemcpyAsync(h_ctl, d_ctl, n_words * 8, hipMemcpyDeviceToHost, e->stream), what.c_str());
    HIP_TRY(hipStreamSynchronize(e->stream), what.c_str());
    if (h_ctl[kSelCtlFlag]) return fail(e, GFT_E_INVALID, std::string(G.who) + ": document offsets descend, or a document of 4 GiB or more");
    return GFT_OK;
}

int doc_gather_overlap(const gft_engine* e, const DocGather& G) { return fail(e, GFT_E_INVALID, std::string(G.who) + ": an output overlaps an input"); }

int doc_gather_copy(gft_engine* e, const DocGather& G, const uint8_t* text, const uint64_t* c_off, const uint64_t* c_src, uint64_t m, uint64_t total,
                    uint8_t* out, uint64_t cap_bytes) {
    if (int rc = select_copy_run(e, text, c_off, c_src, m, total, out, cap_bytes, (std::string(G.word) + "_copy").c_str(),
                                 step(G, "copy kernel launch").c_str()))
        return rc;
    HIP_TRY(hipStreamSynchronize(e->stream), step(G, "copy").c_str());
    return GFT_OK;
}

}  // namespace gft::api
