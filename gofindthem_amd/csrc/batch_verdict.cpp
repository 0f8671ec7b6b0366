// batch_verdict.cpp -- see batch_verdict.hpp
#include "batch_verdict.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>

#include "gft_guard.hpp"

namespace gft {

CtlBlock decode_ctl(const uint64_t w[kCtlWords]) {
    CtlBlock c;
    c.bad = (uint32_t)w[kCtlBad / 8];
    c.cursor = w[kCtlCursor / 8];
    c.total = w[kCtlTotal / 8];
    c.nonascii_bits = (uint32_t)w[kCtlNonascii / 8];
    c.miss_epoch = (uint32_t)(w[kCtlNonascii / 8] >> 32);
    c.n_units = w[kCtlUnits / 8];
    c.text_lo = w[kCtlUnits / 8 + 1];
    c.text_hi = w[kCtlUnits / 8 + 2];
    return c;
}

Judgement judge_deferred(const CtlBlock& c, const ScanLaunch& L) {
    Judgement j;
    BatchVerdict& v = j.verdict;
    v.nonascii_bits = c.nonascii_bits; v.nonascii = c.nonascii_bits != 0;
    v.text_lo = c.text_lo; v.text_hi = c.text_hi;
    v.n_units = c.n_units; v.total = c.total;
    if (single_miss(c, L)) { j.kind = Judgement::again_general; return j; }
    if (c.text_hi < c.text_lo) { j.kind = Judgement::invalid; j.err = "doc_off is not ascending"; return j; }
    // (a k_units_single batch raises its flags to its epoch; what an earlier batch left there is smaller)
    if (L.single ? c.bad == L.epoch : c.bad != 0) {
        j.kind = Judgement::invalid;
        j.err = "doc_off is not ascending, or a document is longer than 4 GiB - 1 bytes (positions are 32-bit)";
        return j;
    }
    // (the DFA kernel's cursor counts matches, the suffix-window kernels' slabs: both must fit the pool the launch had)
    const uint64_t cursor = c.cursor + L.static_slabs;
    if (cursor > L.pool_cap) { j.kind = Judgement::again_grow; j.pool_need = cursor + cursor / 16; }
    else if (c.n_units > L.unit_cap) j.kind = Judgement::again_general;
    return j;
}

void learn(Learned& s, ScanKernel kernel, uint32_t fifo_cap, bool ordered, uint64_t total, uint64_t text_lo, uint64_t text_hi) {
    if (text_hi <= text_lo) return;
    const double per_byte = (double)total / (double)(text_hi - text_lo);
    if (kernel == ScanKernel::scan4) s.scan4_density = std::max(0.002, per_byte);
    if (on_scan2_tables(kernel) && !ordered) {
        // a unit's matches should fit the wave's LDS fifo: a unit of maximal size should fill ~75 % of it (dense
        // dictionaries -> smaller units; results do not depend on the unit size)
        const double want = per_byte > 0 ? 0.75 * fifo_cap / per_byte : (double)kScan2UnitMax;
        const uint32_t um = want >= kScan2UnitMax ? kScan2UnitMax : (uint32_t)want & ~255u;
        s.unit_max = std::max<uint32_t>(512, um);
    }
}

}  // namespace gft

// ---- test hooks (include/gft.h): the functions above and nothing else ------------------------------------------------------
using namespace gft;

extern "C" {

int gft_debug_judge_batch(const uint64_t* ctl_words, int single, uint32_t epoch, uint64_t n_docs, uint64_t unit_cap, uint64_t pool_cap,
                          uint64_t static_slabs, int* kind, uint64_t* pool_need, uint64_t* verdict, char* err_out, uint64_t err_cap) try {
    if (!ctl_words || !kind || !pool_need || !verdict) return GFT_E_INVALID;
    ScanLaunch L;
    L.deferred = true; L.single = single != 0; L.epoch = epoch;
    L.n_docs = n_docs; L.unit_cap = unit_cap; L.pool_cap = pool_cap; L.static_slabs = static_slabs;
    const Judgement j = judge_deferred(decode_ctl(ctl_words), L);
    *kind = (int)j.kind;
    *pool_need = j.pool_need;
    const BatchVerdict& v = j.verdict;
    const uint64_t out[6] = {v.nonascii ? 1u : 0u, v.nonascii_bits, v.text_lo, v.text_hi, v.n_units, v.total};
    memcpy(verdict, out, sizeof out);
    if (err_out && err_cap) { const size_t n = std::min<size_t>(strlen(j.err), err_cap - 1); memcpy(err_out, j.err, n); err_out[n] = 0; }
    return GFT_OK;
} GFT_CATCH(nullptr)

int gft_debug_learn(const char* kernel, uint32_t fifo_cap, int ordered, uint64_t total, uint64_t text_lo, uint64_t text_hi,
                    uint32_t* unit_max, double* scan4_density) try {
    if (!kernel || !unit_max || !scan4_density) return GFT_E_INVALID;
    for (int k = 0; k < 5; k++)
        if (!strcmp(kernel, kScanKernelName[k])) {
            Learned s;
            s.unit_max = *unit_max; s.scan4_density = *scan4_density;
            learn(s, (ScanKernel)k, fifo_cap, ordered != 0, total, text_lo, text_hi);
            *unit_max = s.unit_max; *scan4_density = s.scan4_density;
            return GFT_OK;
        }
    return GFT_E_INVALID;
} GFT_CATCH(nullptr)

}  // extern "C"
