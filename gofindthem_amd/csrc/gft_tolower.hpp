// gft_tolower.hpp -- strings.ToLower on the device (gft_tolower.hip): launchers, the mapping table's host form and the
// walk of the same pieces on the host (tolower_host.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/gft.h"
#include "gft_kernels.hpp"
#include "gft_tolower_piece.hpp"
#include "gft_lowermap_piece.hpp"

namespace gft {

// The two-level table of gft_tolower_piece.hpp, derived from the pairs of unicode_lower.inc (dsl::LowerPairs) the first time
// it is asked for; every engine uploads its own copy once.
struct LowerTableHost {
    std::vector<uint16_t> page;      // [n_pages]: 0 or the page's row of delta
    std::vector<int32_t> delta;      // [(1 + non-identity pages) * 64], row 0 all zero
    LowerTable view() const { return LowerTable{page.data(), delta.data(), (uint32_t)page.size()}; }
};
const LowerTableHost& lower_table_host();

// Does the output (out[0, cap), out_off[0, n_docs]) overlap the input (text[lo, hi), doc_off[0, n_docs])?
bool lower_buffers_overlap(const uint8_t* text, uint64_t lo, uint64_t hi, const uint64_t* doc_off, uint64_t n_docs, const uint8_t* out,
                           uint64_t cap, const uint64_t* out_off);

// gft_to_lower_device on the host, piece by piece through gft_tolower_piece.hpp: unit table as k_unit_count / k_unit_fill
// build it, count per unit, exclusive prefix, write.  blob must be readable 64 bytes past doc_off[n_docs].  Returns a
// gft_status; *total = the lowered size; nothing is stored at or past cap.
int lower_emulate(const uint8_t* blob, const uint64_t* doc_off, uint64_t n_docs, uint8_t* out, uint64_t cap, uint64_t* out_off,
                  uint64_t* total);

// the three passes of gft_tolower.hip on d_units[0, n_units) (T: device pointers)
hipError_t launch_lower_count(const uint8_t* d_text, const uint64_t* d_doc_off, const Unit* d_units, uint64_t n_units, const LowerTable& T,
                              uint32_t* d_unit_cnt, unsigned n_cus, hipStream_t st);
// d_out_off[d] = d_unit_out[d_unit_base[d]], d <= n_docs; *d_bad |= 2 when a document's lower-case form has 4 GiB or more
hipError_t launch_lower_offsets(const uint64_t* d_unit_base, const uint64_t* d_unit_out, uint64_t n_docs, uint64_t* d_out_off,
                                uint32_t* d_bad, hipStream_t st);
hipError_t launch_lower_write(const uint8_t* d_text, const uint64_t* d_doc_off, const Unit* d_units, uint64_t n_units, const LowerTable& T,
                              const uint64_t* d_unit_out, uint8_t* d_out, uint64_t cap, unsigned n_cus, hipStream_t st);

// the walk of launch_lower_write with the table form of the kernel: d_tab[lowermap_slot(..)] = where the piece's output begins
// in its document's lower-case form (gft_lowermap_piece.hpp); d_unit_base: the first unit of every document; text_lo: doc_off[0]
hipError_t launch_lower_table(const uint8_t* d_text, const uint64_t* d_doc_off, const Unit* d_units, uint64_t n_units, const LowerTable& T,
                              const uint64_t* d_unit_base, const uint64_t* d_unit_out, uint64_t text_lo, uint32_t* d_tab, unsigned n_cus,
                              hipStream_t st);

// the unit table as k_unit_count / k_unit_fill build it, on the host: unit_base [n_docs + 1] and the units.  GFT_E_INVALID for
// descending offsets or a document of 4 GiB or more
int lower_units_host(const uint64_t* doc_off, uint64_t n_docs, std::vector<uint64_t>& unit_base, std::vector<Unit>& units);

}  // namespace gft

// for finder_host.cpp: the batch lowered into buffers the engine owns (grown on demand, 64 bytes of slack behind the text),
// enqueued on the engine's stream -- *d_lowered / *d_lowered_off stay valid until the next call of this function on e.
// GFT_E_NOMEM when the device has no room for them.
extern "C" int gft_lower_owned(gft_engine* e, const uint8_t* d_text_blob, const uint64_t* d_doc_off, uint64_t n_docs, const uint8_t** d_lowered,
                    const uint64_t** d_lowered_off);
