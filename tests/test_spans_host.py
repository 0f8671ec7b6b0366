"""Hit spans and redaction on the host (csrc/witness_terms.cpp, spans_host.cpp): gft_debug_witness_terms against a walk over the
parsed trees; gft_debug_hit_spans and gft_debug_redact_spans -- the kernels' walks through gft_spans_piece.hpp -- against the
reference of spans.py on every fixed case and on seeded random batches; the cap protocol into guarded arrays; the refusals; and
that the cases are not vacuous.  All comparisons are exact.  No device needed."""
import numpy as np
import pytest

import spans as S
from gofindthem_amd import _lib
from gofindthem_amd.engine import GftError, hit_spans_host, redact_spans_host, spans_shape, witness_terms_host

GUARD32, GUARD64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5


def walk(c, **kw):
    """gft_debug_hit_spans over the oracle's matches of a case, with the library's own witness table"""
    k = S.compiled(c.exprs, c.fold)
    wo, we = witness_terms_host(k.programs, k.n_terms, k.n_terms + k.n_extra)
    moff, tid, pos = S.matches(c)
    return hit_spans_host(moff, tid, pos, k.term_len, c.pos_end, wo, we, c.rows, len(k.programs), c.row_idx, c.want, **kw)


def lists(total, span_off, start, length, term, n_docs):
    return total, span_off[:n_docs + 1].tolist(), start[:total].tolist(), length[:total].tolist(), term[:total].tolist()


def test_the_shape():
    T, s = spans_shape()
    assert T >= 64 and T % 64 == 0 and s == 64


def test_the_cases_are_not_vacuous():
    assert S.assert_not_vacuous()


@pytest.mark.parametrize("exprs", S.WITNESS_EXPRS, ids=lambda e: "%d: %s" % (len(e), e[-1][:40]))
def test_witness_table_against_the_tree_walk(exprs):
    k = S.compiled(tuple(exprs), False)
    off, expr = witness_terms_host(k.programs, k.n_terms, k.n_terms + k.n_extra)
    ref_off, ref_expr = k.witness_table()
    assert off.tolist() == ref_off.tolist() and expr.tolist() == ref_expr.tolist()
    for t in range(k.n_terms):                                          # ascending, each expression once
        e = expr[int(off[t]):int(off[t + 1])].tolist()
        assert e == sorted(set(e))


def test_witness_table_says_what_the_contract_says():
    def table(exprs):
        k = S.compiled(tuple(exprs), False)
        off, expr = witness_terms_host(k.programs, k.n_terms, k.n_terms + k.n_extra)
        return {k.terms[t].decode(): expr[int(off[t]):int(off[t + 1])].tolist() for t in range(k.n_terms)}
    assert table(['not "a"']) == {"a": []}
    assert table(['not (not "a")']) == {"a": []}                        # a NOT removes, nothing restores
    assert table(['"a" and not ("b" or "c")']) == {"a": [0], "b": [], "c": []}
    assert table(['"a" and "b"', '"c" and not "a"']) == {"a": [0], "b": [0], "c": [1]}
    assert table(['"a" and ("b" or "a")']) == {"a": [0], "b": [0]}
    assert table(['inord("a" and "b")']) == {"a": [0], "b": [0]}
    assert table(['"a" and r"b+"', 'r"c" or "d"']) == {"a": [0], "d": [1]}
    assert table(['("a" and "b") or "c"']) == {"a": [0], "b": [0], "c": [0]}     # no minimal witness
    t = table(['"k" and "u%d"' % i for i in range(70)])
    assert t["k"] == list(range(70)) and all(t["u%d" % i] == [i] for i in range(70))
    for n in (1, 32, 33, 2081):
        assert table(['not "zz"'] * (n - 1) + ['"a"']) == ({"a": [n - 1], "zz": []} if n > 1 else {"a": [0]})


def test_witness_table_refusals_and_cap():
    L = _lib.load()
    import ctypes as C
    UNIT, AND, NOT = 1 << 28, 2 << 28, 4 << 28

    def rc(words, n_slots=2, offs=None):
        w = np.asarray(words or [0], dtype=np.uint32)
        o = np.asarray(offs if offs is not None else [0, len(words)], dtype=np.uint64)
        off = np.zeros(3, dtype=np.uint64)
        needed = C.c_uint64(7)
        return L.gft_debug_witness_terms(w.ctypes.data, o.ctypes.data, len(o) - 1, 2, n_slots, off.ctypes.data, None, 0, C.byref(needed)), needed.value
    assert rc([UNIT | 0, UNIT | 1, AND]) == (0, 2)
    assert rc([UNIT | 0, AND])[0] == _lib.GFT_E_INVALID                 # an operator without its operands
    assert rc([NOT])[0] == _lib.GFT_E_INVALID
    assert rc([UNIT | 0, UNIT | 1])[0] == _lib.GFT_E_INVALID            # two values left
    assert rc([])[0] == _lib.GFT_E_INVALID                              # none
    assert rc([UNIT | 2])[0] == _lib.GFT_E_INVALID                      # no such slot
    assert rc([UNIT | 2], n_slots=3) == (0, 0)                          # an extra slot: no witness
    assert rc([7 << 28])[0] == _lib.GFT_E_INVALID
    assert rc([UNIT | 0], offs=[1, 0])[0] == _lib.GFT_E_INVALID
    # the cap: entries at and past it stay untouched, the offsets are complete
    k = S.compiled(tuple('"k" and "u%d"' % i for i in range(70)), False)
    words = np.asarray([w for p in k.programs for w in p], dtype=np.uint32)
    poff = np.cumsum([0] + [len(p) for p in k.programs]).astype(np.uint64)
    off = np.zeros(k.n_terms + 1, dtype=np.uint64)
    expr = np.full(20, GUARD32, dtype=np.uint32)
    needed = C.c_uint64(0)
    assert L.gft_debug_witness_terms(words.ctypes.data, poff.ctypes.data, 70, k.n_terms, k.n_terms, off.ctypes.data, expr.ctypes.data, 10, C.byref(needed)) == 0
    ref_off, ref_expr = k.witness_table()
    assert needed.value == 140 and off.tolist() == ref_off.tolist() and expr[:10].tolist() == ref_expr[:10].tolist() and (expr[10:] == GUARD32).all()


@pytest.mark.parametrize("c", S.fixed_cases(), ids=lambda c: c.name[:60])
def test_fixed_cases(c):
    assert lists(*walk(c), len(c.docs)) == S.expected()[c.name]


def test_random_batches():
    for c in S.random_cases():
        assert lists(*walk(c), len(c.docs)) == S.expected()[c.name], c.name


def test_cap_protocol():
    c = next(c for c in S.fixed_cases() if c.name == "mixed documents, rows permuted")
    total, off, start, length, term = S.expected()[c.name]
    n = len(c.docs)
    for cap in (0, 1, total - 1, total, total + 3):
        t, so, a, b, d = walk(c, cap=cap, guard=8)
        m = min(cap, total)
        assert t == total and so[:n + 1].tolist() == off and (so[n + 1:] == GUARD64).all(), cap
        assert a[:m].tolist() == start[:m] and b[:m].tolist() == length[:m] and d[:m].tolist() == term[:m], cap
        assert (a[m:] == GUARD32).all() and (b[m:] == GUARD32).all() and (d[m:] == GUARD32).all(), cap
    # len and term are optional, each on its own
    t, so, a, b, d = walk(c, with_len=False)
    assert b is None and a[:total].tolist() == start and d[:total].tolist() == term
    t, so, a, b, d = walk(c, with_term=False)
    assert d is None and a[:total].tolist() == start and b[:total].tolist() == length


def test_hit_spans_refusals():
    c = next(c for c in S.fixed_cases() if c.name == "mixed documents, identity")
    k = S.compiled(c.exprs, c.fold)
    wo, we = witness_terms_host(k.programs, k.n_terms, k.n_terms)
    moff, tid, pos = S.matches(c)
    L = _lib.load()
    import ctypes as C
    total = C.c_uint64(5)
    n = len(c.docs)
    so = np.zeros(n + 1, dtype=np.uint64)

    def call(match_off=moff, span_off=so, start=None, cap=0):
        return L.gft_debug_hit_spans(match_off.ctypes.data, tid.ctypes.data, pos.ctypes.data, n, k.term_len.ctypes.data, 0, wo.ctypes.data, we.ctypes.data,
                                     c.rows.ctypes.data, 3, None, None, span_off.ctypes.data if span_off is not None else None,
                                     start.ctypes.data if start is not None else None, None, None, cap, C.byref(total))
    assert call() == 0 and total.value == S.expected()[c.name][0]
    assert call(cap=4) == _lib.GFT_E_INVALID and total.value == 0       # a cap without its array
    bad = moff.copy()
    bad[3], bad[4] = bad[4] + 1, bad[3]
    assert call(match_off=bad) == _lib.GFT_E_INVALID                    # offsets that descend
    assert call(span_off=moff) == _lib.GFT_E_INVALID                    # an output that is an input
    both = np.zeros(max(n + 1, 16) * 2, dtype=np.uint32)
    assert call(span_off=both.view(np.uint64), start=both, cap=4) == _lib.GFT_E_INVALID      # two outputs that overlap
    assert call() == 0
    # no documents, no expressions
    assert L.gft_debug_hit_spans(None, None, None, 0, None, 0, None, None, None, 0, None, None, so.ctypes.data, None, None, None, 0, C.byref(total)) == 0
    assert total.value == 0 and so[0] == 0
    none_off = np.zeros(k.n_terms + 1, dtype=np.uint64)
    assert L.gft_debug_hit_spans(moff.ctypes.data, tid.ctypes.data, pos.ctypes.data, n, k.term_len.ctypes.data, 0, none_off.ctypes.data, None, None, 0,
                                 None, None, so.ctypes.data, None, None, None, 0, C.byref(total)) == 0
    assert total.value == 0 and not so.any()


@pytest.mark.parametrize("f", S.fill_cases(), ids=lambda f: f.name[:60])
def test_redaction(f):
    if not f.ok:
        with pytest.raises(GftError) as ei:
            redact_spans_host(f.blob, f.doc_off, f.span_off, f.start, f.length, f.mask)
        assert ei.value.code == _lib.GFT_E_INVALID
        # nothing was written: the walk works on a copy here, so ask the C call itself
        a = f.blob.copy()
        rc = _lib.load().gft_debug_redact_spans(a.ctypes.data, f.doc_off.ctypes.data, len(f.doc_off) - 1, f.span_off.ctypes.data, f.start.ctypes.data,
                                                f.length.ctypes.data, f.mask)
        assert rc == _lib.GFT_E_INVALID and np.array_equal(a, f.blob)
        return
    out = redact_spans_host(f.blob, f.doc_off, f.span_off, f.start, f.length, f.mask)
    assert out.tobytes() == S.redact_reference(f)
    # (random bytes everywhere and none of them the mask: the masked bytes are exactly the spans' bytes)
    assert int((out == f.mask).sum()) == len({int(f.doc_off[d]) + int(f.start[s]) + j for d in range(len(f.doc_off) - 1)
                                              for s in range(int(f.span_off[d]), int(f.span_off[d + 1])) for j in range(int(f.length[s]))})


def test_redaction_refusals():
    f = S.fill_cases()[0]
    L = _lib.load()
    a = f.blob.copy()
    args = (a.ctypes.data, f.doc_off.ctypes.data, len(f.doc_off) - 1, f.span_off.ctypes.data, f.start.ctypes.data, f.length.ctypes.data)
    assert L.gft_debug_redact_spans(*args, 256) == _lib.GFT_E_INVALID and np.array_equal(a, f.blob)
    down = f.span_off.copy()
    down[0], down[-1] = down[-1], 0
    assert L.gft_debug_redact_spans(args[0], args[1], args[2], down.ctypes.data, args[4], args[5], 42) == _lib.GFT_E_INVALID and np.array_equal(a, f.blob)
    assert L.gft_debug_redact_spans(None, None, 0, None, None, None, 42) == 0
    assert L.gft_debug_redact_spans(*args, 42) == 0 and a.tobytes() == S.redact_reference(f)


def test_spans_of_a_hit_then_the_redaction_of_them():
    """the two walks together: the spans of a case, masked in its text, are the reference's masked text"""
    c = next(c for c in S.fixed_cases() if c.name.startswith("abc, bcd and abcd in xabcdx, POS_END"))
    total, span_off, start, length, term = S.expected()[c.name]
    blob, off = S.packed(c)
    out = redact_spans_host(blob.tobytes(), off, span_off, start, length, ord("#"))
    assert out.tobytes() == b"######" b"####" b"###" b"z###" b"###z"
