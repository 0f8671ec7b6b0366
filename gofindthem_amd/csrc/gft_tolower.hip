// gft_tolower.hip -- strings.ToLower (finder/finder.go:140-142) over a batch on the device, gfx950 / wave64: what the finder
// runs for a batch whose text the scan kernels' A-Z fold does not cover (gft_last_nonascii) instead of sending it to the host.
//
//   (text, doc_off [n_docs + 1])  ->  (out, out_off [n_docs + 1]): every document's lower-case form, concatenated
//
//   k_lower<kLowerCount>  output bytes per work unit {doc, lo, hi} (the unit table of k_unit_count / k_unit_fill)  -> unit_cnt
//   (k_scan_* of gft_kernels.hip: unit_cnt -> unit_out)
//   k_lower_offsets   out_off[d] = unit_out[first unit of document d]
//   k_lower<kLowerWrite>  the same walk again: prefix of the pieces' lengths over the wave (DPP), carried from trip to trip,
//                     every lane writes its piece at unit_out[unit] + prefix
//   k_lower<kLowerTable>  that walk for gft_map_spans_to_source_device (gft_lowermap.hip): instead of the piece's bytes every
//                     lane stores WHERE its piece's output begins in its document's lower-case form, one uint32 per piece
//
// A wave owns a unit and walks it in trips of 1 KiB, a lane owns 16 bytes of a trip; what a piece becomes is decided by
// gft_tolower_piece.hpp, which the host compiles too.  Lengths change (U+0130 shrinks, U+023A grows, an invalid byte becomes
// three), hence the two passes.  Memory bound: two reads of the text and one write; the mapping table (17 KB) stays in cache.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gft_kernels.hpp"
#include "gft_tolower.hpp"
#include "gft_wave_dev.hpp"

namespace gft {

namespace {

constexpr uint32_t kLowerBlock = 256;       // 4 waves

struct LowerParams {
    const uint8_t* text;
    const uint64_t* doc_off;
    const Unit* units;
    uint64_t n_units;
    LowerTable T;
    uint32_t* unit_cnt;             // count pass
    const uint64_t* unit_out;       // write pass
    uint8_t* out;
    uint64_t cap;
    const uint64_t* unit_base;      // table pass: the first unit of every document
    uint32_t* tab;                  //             the pieces' offsets, a slot each (lowermap_slot)
    uint64_t text_lo;               //             doc_off[0]
};

enum : int { kLowerCount = 0, kLowerWrite = 1, kLowerTable = 2 };


template <int MODE>
__global__ void __launch_bounds__(kLowerBlock) k_lower(const LowerParams P) {
    constexpr bool WRITE = MODE != kLowerCount;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * kLowerBlock + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * kLowerBlock) >> 6;
    for (uint64_t u = wave; u < P.n_units; u += n_waves) {
        const Unit un = P.units[u];
        const uint64_t doc_abs = P.doc_off[un.doc];
        const uint64_t doc_len = P.doc_off[un.doc + 1] - doc_abs;
        uint64_t carry = WRITE ? P.unit_out[u] : 0;
        uint64_t slot = 0;
        if (MODE == kLowerTable) {
            carry -= P.unit_out[P.unit_base[un.doc]];                            // relative to the document's lowered start
            slot = lowermap_slot(doc_abs - P.text_lo + un.lo, u) + lane;
        }
        uint32_t sum = 0;
        for (uint64_t base = un.lo; base < un.hi; base += kLowerChunk) {       // (the same in every lane)
            const uint64_t o = base + lane * kLowerPiece;                       // the piece's offset in its document
            const uint32_t n = o < un.hi ? (uint32_t)std::min<uint64_t>(kLowerPiece, un.hi - o) : 0u;
            LowerWin w;
            uint32_t len = 0;
            if (n) {
                tolower_load_piece(P.text + doc_abs + o, o < 3 ? (uint32_t)o : 3u, doc_len - o, w);
                len = tolower_piece<false>(P.T, w, n, nullptr, 0, 0);
            }
            if (!WRITE) {
                sum += len;
            } else {
                const uint32_t incl = wave_incl_scan(len);
                if (MODE == kLowerTable) {
                    if (n) P.tab[slot + (base - un.lo) / kLowerPiece] = (uint32_t)(carry + (incl - len));
                } else if (n) {
                    tolower_piece<true>(P.T, w, n, P.out, carry + (incl - len), P.cap);
                }
                carry += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            }
        }
        if (!WRITE) {
            sum = wave_incl_scan(sum);
            if (lane == 63) P.unit_cnt[u] = sum;
        }
    }
}

// out_off[d] = unit_out[unit_base[d]] (every document has a unit; unit_base[n_docs] = n_units, unit_out[n_units] = the total);
// *bad |= 2 when a document's lower-case form has 4 GiB or more
__global__ void __launch_bounds__(256) k_lower_offsets(const uint64_t* __restrict__ unit_base, const uint64_t* __restrict__ unit_out,
                                                       uint64_t n_docs, uint64_t* __restrict__ out_off, uint32_t* __restrict__ bad) {
    const uint64_t d = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d > n_docs) return;
    const uint64_t a = unit_out[unit_base[d]];
    out_off[d] = a;
    if (d < n_docs && unit_out[unit_base[d + 1]] - a > 0xFFFFFFFFull) atomicOr(bad, 2u);
}

unsigned lower_grid(uint64_t n_units, unsigned n_cus) {
    const uint64_t blocks = (n_units + kLowerBlock / 64 - 1) / (kLowerBlock / 64);
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(blocks, (uint64_t)std::max(n_cus, 1u) * 8));   // 32 waves per CU
}

}  // namespace

hipError_t launch_lower_count(const uint8_t* d_text, const uint64_t* d_doc_off, const Unit* d_units, uint64_t n_units, const LowerTable& T,
                              uint32_t* d_unit_cnt, unsigned n_cus, hipStream_t st) {
    if (!n_units) return hipSuccess;
    LowerParams P{};
    P.text = d_text; P.doc_off = d_doc_off; P.units = d_units; P.n_units = n_units; P.T = T;
    P.unit_cnt = d_unit_cnt;
    k_lower<kLowerCount><<<dim3(lower_grid(n_units, n_cus)), dim3(kLowerBlock), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_lower_offsets(const uint64_t* d_unit_base, const uint64_t* d_unit_out, uint64_t n_docs, uint64_t* d_out_off,
                                uint32_t* d_bad, hipStream_t st) {
    k_lower_offsets<<<dim3((unsigned)((n_docs + 1 + 255) / 256)), dim3(256), 0, st>>>(d_unit_base, d_unit_out, n_docs, d_out_off, d_bad);
    return hipGetLastError();
}

hipError_t launch_lower_write(const uint8_t* d_text, const uint64_t* d_doc_off, const Unit* d_units, uint64_t n_units, const LowerTable& T,
                              const uint64_t* d_unit_out, uint8_t* d_out, uint64_t cap, unsigned n_cus, hipStream_t st) {
    if (!n_units || !cap) return hipSuccess;
    LowerParams P{};
    P.text = d_text; P.doc_off = d_doc_off; P.units = d_units; P.n_units = n_units; P.T = T;
    P.unit_out = d_unit_out; P.out = d_out; P.cap = cap;
    k_lower<kLowerWrite><<<dim3(lower_grid(n_units, n_cus)), dim3(kLowerBlock), 0, st>>>(P);
    return hipGetLastError();
}

hipError_t launch_lower_table(const uint8_t* d_text, const uint64_t* d_doc_off, const Unit* d_units, uint64_t n_units, const LowerTable& T,
                              const uint64_t* d_unit_base, const uint64_t* d_unit_out, uint64_t text_lo, uint32_t* d_tab, unsigned n_cus,
                              hipStream_t st) {
    if (!n_units) return hipSuccess;
    LowerParams P{};
    P.text = d_text; P.doc_off = d_doc_off; P.units = d_units; P.n_units = n_units; P.T = T;
    P.unit_out = d_unit_out; P.unit_base = d_unit_base; P.tab = d_tab; P.text_lo = text_lo;
    k_lower<kLowerTable><<<dim3(lower_grid(n_units, n_cus)), dim3(kLowerBlock), 0, st>>>(P);
    return hipGetLastError();
}

}  // namespace gft
