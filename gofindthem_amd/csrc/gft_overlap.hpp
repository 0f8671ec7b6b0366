// gft_overlap.hpp -- may a call write where it was told to: the one test of a call's output ranges against its input ranges and
// against each other.  No HIP.  Every call writes down its own two lists (<call>_buffers_overlap in its header) and hands them over.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace gft {

struct ByteRange {
    const void* p;
    uint64_t n;
};

// two byte ranges meet (a null pointer or an empty range meets nothing)
inline bool ranges_meet(const ByteRange& a, const ByteRange& b) {
    const uintptr_t x = (uintptr_t)a.p, y = (uintptr_t)b.p;
    return a.p && b.p && a.n && b.n && x < y + b.n && y < x + a.n;
}

// an output meets an input, or a later output
inline bool outputs_overlap(const ByteRange* outs, size_t n_out, const ByteRange* ins, size_t n_in) {
    for (size_t o = 0; o < n_out; o++) {
        for (size_t i = 0; i < n_in; i++)
            if (ranges_meet(outs[o], ins[i])) return true;
        for (size_t p = o + 1; p < n_out; p++)
            if (ranges_meet(outs[o], outs[p])) return true;
    }
    return false;
}
template <size_t NO, size_t NI>
inline bool outputs_overlap(const ByteRange (&outs)[NO], const ByteRange (&ins)[NI]) { return outputs_overlap(outs, NO, ins, NI); }

}  // namespace gft
