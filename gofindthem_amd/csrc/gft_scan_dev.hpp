// gft_scan_dev.hpp -- the device kit of the suffix-window scan kernels, shared by the scan2 family (gft_scan2_dev.hpp:
// k_scan5, k_scan2, k_scan4) and the stride-2 kernel (gft_scan3.hip: k_scan3): unaligned text loads around a flagged
// position with their blob-start and blob-end forms, ASCII folding, bucket slots, the deferred-entry list and the compare
// of a long term's head against the text.
// Inclusion convention (gft_scan2_dev.hpp's): included inside namespace gft { namespace { ... } } of a .hip file, after
// gft_kernels.hpp and gft_wave_dev.hpp.  The includer defines, in front of the include,
//   constexpr int kFrontWords   the dwords of Front that its slots hold and front_fold_upto folds (scan2: 5, scan3: 4)
// and, wherever it likes, its own one-line KARG(field) over karg_field.  The text loads are templates on the includer's
// context type C, of which they read  dbase, doc_abs, near0, near24, near_end, P.text_bytes, P.fold  and the type
// C::Params (the kernel's parameter block, for the kernarg offsets of term_blob and term_off).
#pragma once
struct __attribute__((packed, aligned(1))) U32u { uint32_t v; };
struct __attribute__((packed, aligned(1))) U128u { uint32_t x, y, z, w; };
struct __attribute__((packed, aligned(1))) U64u { uint32_t lo, hi; };

// a * b + c on 24-bit operands: one full-rate instruction (the compiler's own choice is v_mul_lo_u32 / v_mad_u64_u32);
// the wave-uniform multiplier comes straight from a scalar register (no v_mov to materialise it)
__device__ __forceinline__ uint32_t mad24s(uint32_t a, uint32_t sb, uint32_t c) {
    uint32_t d;
    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(d) : "v"(a), "s"(sb), "v"(c));
    return d;
}
// LDS tables at fixed addresses (the kernel's only LDS object is the dynamic array, which starts at 0; checked at
// kernel entry): constant bases fold into the ds_read offset field
typedef __attribute__((address_space(3))) const uint8_t lds_u8;
typedef __attribute__((address_space(3))) const uint32_t lds_u32;
__device__ __forceinline__ uint32_t load_u32_unaligned(const uint8_t* p) { return reinterpret_cast<const U32u*>(p)->v; }

// Kernel arguments that are needed once per unit or less (output buffers, tables of the rare paths) are read from the
// kernarg segment where they are used instead of living in scalar registers for the whole kernel: the unit loop keeps
// more values alive than there are SGPRs, and every spilled one costs VALU slots (v_writelane / v_readlane).  The asm
// makes the address opaque, so the load can be neither merged with the preloaded arguments nor hoisted.
typedef __attribute__((address_space(4))) const uint8_t karg_u8;
template <class T>
__device__ __forceinline__ T karg_field(uint32_t off) {
    karg_u8* ka = (karg_u8*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));
    return *(__attribute__((address_space(4))) const T*)(ka + off);
}

// ASCII lower-casing of four packed bytes (finder/finder.go:140-142 for ASCII text)
__device__ __forceinline__ uint32_t fold4(uint32_t w) {
    const uint32_t h = w & 0x7F7F7F7Fu;
    const uint32_t ge_a = h + 0x3F3F3F3Fu;          // bit 7 set where byte >= 'A'
    const uint32_t gt_z = h + 0x25252525u;          // bit 7 set where byte >  'Z'
    const uint32_t up = ge_a & ~gt_z & ~w & 0x80808080u;
    return w | (up >> 2);
}
__device__ __forceinline__ uint32_t fold1(uint32_t b) { return (b - 'A' < 26u) ? b + 32 : b; }

// ---- text around a flagged position p ---------------------------------------------------------------------------------------
// one 8-byte load brings the window (bytes p-3..p) and the 4 bytes in front of it (p-7..p-4).
// Positions before the document start need no special casing here: the bytes there (the previous document's, or
// zeros in front of the blob) can only change keys of windows that reach across the start, and every term such a
// window may name is longer than p + 1 and is dropped by the length check at emission.
struct Text8 { uint32_t tw, w; };
template <class C>
__device__ __forceinline__ Text8 cand_load_slow(const C& c, uint32_t p) {   // within 7 bytes of the blob start
    Text8 t{0, 0};
    const uint64_t ab = c.doc_abs + p;
    if (ab >= 7) {
        const U64u v = *reinterpret_cast<const U64u*>(c.dbase + (int64_t)p - 7);
        t.tw = v.lo; t.w = v.hi;
    } else {
        for (uint32_t i = 0; i <= (uint32_t)ab; i++) {        // oldest byte first; byte p ends up on top of w
            t.tw = t.tw >> 8 | t.w << 24;
            t.w = t.w >> 8 | (uint32_t)c.dbase[(int64_t)p - (int64_t)ab + i] << 24;
        }
    }
    return t;
}
template <class C>
__device__ __forceinline__ Text8 cand_load(const C& c, uint32_t p) {
    if (__builtin_expect(c.near0, 0)) return cand_load_slow(c, p);        // wave-uniform: first document of the blob
    const U64u v = *reinterpret_cast<const U64u*>(c.dbase + (int64_t)p - 7);
    return Text8{v.lo, v.hi};
}
// the 20 bytes in front of the window as the slots store them, f[k] = text[p-7-4k .. p-4-4k]
struct Front { uint32_t f[5]; };
template <class C>
__device__ __forceinline__ Front front_load(const C& c, uint32_t p, uint32_t tw) {
    Front t;
    t.f[0] = tw;
    if (__builtin_expect(c.near24, 0)) {                      // wave-uniform: first document of the blob
        const uint64_t ab = c.doc_abs + p;
#pragma unroll
        for (int k = 1; k < 5; k++) {
            uint32_t v = 0;
            for (int b = 0; b < 4; b++)
                if (ab >= (uint64_t)(7 + 4 * k - b)) v |= (uint32_t)c.dbase[(int64_t)p - 7 - 4 * k + b] << (8 * b);
            t.f[k] = v;
        }
    } else {
        const U128u v = *reinterpret_cast<const U128u*>(c.dbase + (int64_t)p - 23);
        t.f[4] = v.x; t.f[3] = v.y; t.f[2] = v.z; t.f[1] = v.w;
    }
    return t;
}
// fold the first kmax dwords of t that are not folded yet (`done` = how many are; wave-uniform)
__device__ __forceinline__ void front_fold_upto(Front& t, uint32_t& done, uint32_t kmax) {
#pragma unroll
    for (int k = 0; k < kFrontWords; k++)
        if ((uint32_t)k >= done && (uint32_t)k < kmax) t.f[k] = fold4(t.f[k]);
    done = kmax > done ? kmax : done;
}
// the (up to) four bytes behind position p, text[p+1 .. p+4], for the tails of shifted terms; bytes past the blob end
// read as zero (a tail that reached there would end outside the unit and is dropped by the range check anyway)
template <class C>
__device__ __forceinline__ uint32_t tail_load(const C& c, uint32_t p) {
    if (__builtin_expect(c.near_end, 0)) {
        uint32_t v = 0;
        for (uint32_t b = 0; b < 4; b++)
            if (c.doc_abs + p + 1 + b < c.P.text_bytes) v |= (uint32_t)c.dbase[(uint64_t)p + 1 + b] << (8 * b);
        return v;
    }
    return load_u32_unaligned(c.dbase + (uint64_t)p + 1);
}

// ---- bucket table ------------------------------------------------------------------------------------------------------------
struct Slot { uint4 a, b; };      // a = {key, info, len, front[0]}, b = the rest of the front, the tail, the window: the includer's layout
__device__ __forceinline__ Slot slot_load(const Scan2Slot* s) {
    const uint4* q = reinterpret_cast<const uint4*>(s);
    return Slot{q[0], q[1]};
}
// both candidate slots of key x -> the one that holds it; false: no term ends with this window
__device__ __forceinline__ bool slot_pick(uint32_t x, const Slot& s0, const Slot& s1, Slot& out) {
    const bool use1 = s1.a.x == x;
    out.a = use1 ? s1.a : s0.a;
    out.b = use1 ? s1.b : s0.b;
    return use1 || s0.a.x == x;
}

// A term longer than the `inl` bytes its slot holds, whose window ends at p: the first L - inl bytes of term `term`
// against text[p+1-L .. p-inl], four bytes at a time from the end; term_blob carries 4 bytes of slack in front of every
// term, the text side needs 3 bytes of slack before the match (byte by byte where the blob start is nearer than that)
template <class C>
__device__ __forceinline__ bool term_head_ok(const C& c, uint32_t p, uint32_t L, uint32_t inl, uint32_t term) {
    typedef typename C::Params Params;
    const Params& P = c.P;
    const uint8_t* tb = karg_field<decltype(Params::term_blob)>((uint32_t)offsetof(Params, term_blob)) +
                        karg_field<decltype(Params::term_off)>((uint32_t)offsetof(Params, term_off))[term];
    const uint8_t* tp = c.dbase + (int64_t)p + 1 - L;
    const uint32_t n = L - inl;
    bool ok = true;
    if (c.doc_abs + p + 1 - L >= 3) {
        uint32_t j = 0, d2 = 0;      // (P named up front and j declared first: inlined, the loop then compiles to the code it had in place)
        for (; j * 4 < n; j++) {
            const int32_t at = (int32_t)n - 4 - (int32_t)(j * 4);       // may be -1..-3 for the last chunk
            uint32_t tv = load_u32_unaligned(tp + at);
            const uint32_t wv = load_u32_unaligned(tb + at);
            if (P.fold) tv = fold4(tv);
            const uint32_t mask = at >= 0 ? 0xFFFFFFFFu : 0xFFFFFFFFu << (8 * (uint32_t)(-at));
            d2 |= (tv ^ wv) & mask;
        }
        ok = d2 == 0;
    } else {
        for (uint32_t i = 0; i < n && ok; i++) {
            uint32_t b = tp[i];
            if (P.fold) b = fold1(b);
            ok = b == tb[i];
        }
    }
    return ok;
}

// A wave's deferred bucket entries: {candidate, index into `more`} pairs parked in LDS so that the entries of multi-term
// buckets are verified densely (64 distinct entries per trip) instead of one round per bucket depth.
struct Deferred { uint2* list; uint32_t cap, n; };
