"""The families of inord_trees.py on the CPU: the product's host solver (csrc/host_solve.cpp behind gft_debug_host_solve)
against the oracle on every (expression, document) pair -- two independent CPU implementations on shapes that
test_host_solve.py never draws: wide OR groups, the depth edges, real scan positions of overlapping terms, caller-supplied
matches -- and the conditions that keep the GPU module (test_gpu_inord_trees.py: same seeds, trees and documents) from
passing vacuously, judged on the oracle's bitmap alone."""
import ctypes as C

import numpy as np
import pytest

import inord_trees as T
from gofindthem_amd import _lib

FAMILY_NAMES = sorted(T.FAMILIES)


def _doc_maps(fam, pos_mode):
    """per document: (slots u32, offsets u64, positions i64) of the solver map -- the scan's positions of every term that
    occurs, then the caller's matches of every extra literal that occurs"""
    o = fam.oracle(pos_mode)
    blob, off = fam.packed()
    moff, tid, pos = o.scan(blob, off)
    out = []
    for d in range(len(fam.texts)):
        m = {}
        for i in range(int(moff[d]), int(moff[d + 1])):
            m.setdefault(int(tid[i]), []).append(int(pos[i]))
        for lit, p in fam.extra[d]:
            m.setdefault(len(fam.terms) + fam.extra_lits.index(lit), []).append(p)
        keys = list(m)
        offs = np.zeros(len(keys) + 1, np.uint64)
        offs[1:] = np.cumsum([len(m[k]) for k in keys])
        out.append((np.asarray(keys or [0], np.uint32), offs, np.asarray([p for k in keys for p in m[k]] + [0], np.int64), len(keys)))
    return out


@pytest.mark.parametrize("pos_mode", T.POS_MODES, ids=["start", "end"])
@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_host_solver_equals_the_oracle(name, pos_mode):
    fam = T.FAMILIES[name]()
    L = _lib.load()
    want = fam.truth(pos_mode)
    maps = _doc_maps(fam, pos_mode)
    out = C.c_int(-1)
    for i, words in enumerate(fam.programs()):
        w = np.asarray(words, np.uint32)
        for d, (slots, offs, pos, n) in enumerate(maps):
            rc = L.gft_debug_host_solve(w.ctypes.data, len(w), slots.ctypes.data, offs.ctypes.data, pos.ctypes.data, n, C.byref(out))
            assert rc == 0
            assert bool(out.value) == bool(want[d, i]), (fam.exprs[i][:200], fam.texts[d][:80], fam.extra[d])


@pytest.mark.parametrize("pos_mode", T.POS_MODES, ids=["start", "end"])
@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_family_is_not_vacuous(name, pos_mode):
    """at least 10 % of the (INORD expression, document) pairs true and 10 % false; and where presence alone would say true
    (every inord(X) replaced by X), the INORD form says false in at least 10 %: the order of the occurrences decides"""
    t, f, order = T.FAMILIES[name]().coverage(pos_mode)
    print("%s: true %.3f false %.3f present-but-not-in-order %.3f" % (name, t, f, order))
    assert t >= 0.10 and f >= 0.10 and order >= 0.10


@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_stated_classes(name):
    """the groups are narrow / wide / beyond the device's limits on purpose: the family's statement against the restated
    pair arithmetic"""
    fam = T.FAMILIES[name]()
    got = [T.classify(w) for w in fam.programs()]
    for e, g, c in zip(fam.exprs, got, fam.classes):
        assert c is None or g == c, (e[:200], g, c)
    if name == "limits":
        stats = [T.group_stats(w)[0][0] for w in fam.programs()[:10]]
        assert [a for a, _ in stats[:3]] == [63, 64, 65]
        assert [d for _, d in stats[4:8]] == [32, 33, 64, 65]
        assert [a for a, _ in stats[8:10]] == [8192, 8193]
        assert got.count(T.HOST) == 3
    if name in ("wide", "scratch"):
        assert all(len(w) > 128 for w in fam.programs())         # several rounds of 128 public words


def test_pair_arithmetic_on_hand_counted_groups():
    ws = T.words_of
    assert T.group_stats(ws('inord("a" and "b" and "c")')) == ([(2, 2)], 2)                 # AND leaves the right operand's count
    assert T.group_stats(ws('inord("a" and ("b" and "c"))')) == ([(3, 3)], 3)
    assert T.group_stats(ws('inord(("a" or "b" or "c") and ("d" or "e"))')) == ([(5, 3)], 3)   # OR: the sum
    assert T.group_stats(ws('"x" and not (inord(("a" or "b") and "c")) and inord("d")')) == ([(3, 2), (1, 1)], 3)
    assert T.classify(ws('inord("a" and "b")')) == T.NARROW


def test_named_rows_against_the_oracle():
    """the hand-derived truth values of the quirk rows (dsl/expression.go:66-142, 175-189) are the oracle's"""
    for name in ("narrow", "extra"):
        fam = T.FAMILIES[name]()
        assert fam.named
        for e, d, at_start, at_end in fam.named:
            for pos_mode, v in ((T.POS_START, at_start), (T.POS_END, at_end)):
                assert bool(fam.truth(pos_mode)[d, e]) is v, (fam.exprs[e], fam.texts[d], fam.extra[d], pos_mode)


def test_long_documents_cover_both_layouts():
    """documents on either side of the 8-unit switch (units are at most 8 192 bytes), terms of 2 to 40 bytes, filler that
    occurs in no term"""
    fam = T.family_long()
    sizes = sorted({len(t) for t in fam.texts})
    assert sizes == list(T.LONG_SIZES) and sizes[0] <= 7 * 8192 < 8 * 8192 < sizes[2]
    assert {len(t) for t in fam.terms} >= {2, 3, 4, 40} and not any(c in b". " for t in fam.terms for c in t)
