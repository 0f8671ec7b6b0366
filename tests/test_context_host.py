"""Context lines round the documents that matched -- the host half: gft_debug_context_docs -- the kernels' walk
(csrc/gft_context_piece.hpp) tile by tile on the host -- against the reference of context_docs.py on every fixed and random case, its
identity with the select at before = after = 0, the cap protocol with guard patterns behind the three caps, the refusals, and
Finder.ContextLines on a finder that stays off the device route.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import context_docs as X
import select_docs as S
from gofindthem_amd import _lib
from gofindthem_amd.engine import GftError, context_docs_host, context_shape, select_docs_host
from gofindthem_amd.finder import Finder, Match, PyRegexpEngine, SubstringEngine

GUARD8, GUARD64 = 0xA5, 0xA5A5A5A5A5A5A5A5
NAMES = ("gft_context_docs_device", "gft_debug_context_docs", "gft_debug_context_shape", "gft_finder_context_docs_device")


def test_symbols_and_shape():
    L = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gft.h")).read()
    for name in NAMES:
        assert hasattr(L, name) and name in _lib.SYMBOLS
        assert re.search(r"\b%s\(" % name, header)
    tile, carry, spine = context_shape()
    assert tile == 64 and carry >= 2 and spine >= 2


def test_the_reference_on_the_contract_examples():
    """the reference itself, on cases small enough to read: column 0, documents a, b, c, d, e, f, g, h -- c and g hit"""
    off = list(range(9))
    rows = np.zeros((8, 1), dtype=np.uint32)
    rows[[2, 6], 0] = 1
    ref = lambda b, a, fence=None, also=None, mode="any": X.reference(b"abcdefgh", off, rows, 1, None, mode, also, b, a, fence)   # noqa: E731
    assert ref(0, 0) == (b"cg", [0, 1, 2], [2, 6], [1, 1], [0, 1, 2])
    assert ref(1, 0) == (b"bcfg", [0, 1, 2, 3, 4], [1, 2, 5, 6], [0, 1, 0, 1], [0, 2, 4])
    assert ref(0, 2) == (b"cdegh", [0, 1, 2, 3, 4, 5], [2, 3, 4, 6, 7], [1, 0, 0, 1, 0], [0, 3, 5])
    assert ref(1, 2)[2:] == ([1, 2, 3, 4, 5, 6, 7], [0, 1, 0, 0, 0, 1, 0], [0, 7])                  # the contexts touch: one group
    assert ref(X.U64, X.U64)[2] == list(range(8))
    fence = [0, 0, 0, 1, 0, 0, 0, 0]                                                                # nothing crosses between c and d
    assert ref(1, 2, fence)[2:] == ([1, 2, 5, 6, 7], [0, 1, 0, 1, 0], [0, 2, 5])
    assert ref(X.U64, X.U64, fence)[2:] == (list(range(8)), [0, 0, 1, 0, 0, 0, 1, 0], [0, 3, 8])      # a fence splits a run
    assert ref(1, 1, [9, 0, 1, 0, 0, 0, 0, 0])[2:] == ([2, 3, 5, 6, 7], [1, 0, 0, 1, 0], [0, 2, 5])   # a fence on the hit
    assert ref(1, 0, None, [0, 0, 0, 0, 1, 0, 0, 0])[2:] == ([1, 2, 3, 4, 5, 6], [0, 1, 0, 1, 0, 1], [0, 6])
    assert ref(0, 1, None, None, "none")[2:] == (list(range(8)), [1, 1, 0, 1, 1, 1, 0, 1], [0, 8])     # grep -v -A1


def test_the_cases_are_not_vacuous():
    told = X.assert_not_vacuous()
    assert set(told) == set(X.WRONG)
    T, CB, SPINE = context_shape()
    assert len(X.random_cases()) == 200 and max(len(c.doc_off) for c in X.random_cases()) <= 701
    assert max(len(c.doc_off) for c in X.fixed_cases()) > SPINE * T * CB                          # more than a trip of the spine
    assert {c.before for c in X.random_cases()} | {c.after for c in X.random_cases()} == set(X.REACHES)


def check(c, want_result, shift=0):
    m, hits, groups, total, out, out_off, doc_idx, kind, group_off = context_docs_host(
        c.blob, c.doc_off, c.rows, c.n_cols, c.want, c.mode, c.also, c.before, c.after, c.fence, guard=16, out_shift=shift)
    data, off, idx, kd, go = want_result
    assert (m, hits, groups, total) == (len(idx), sum(kd), len(go) - 1, len(data)), c.name
    assert out[:total].tobytes() == data, c.name
    assert out_off[:m + 1].tolist() == off and doc_idx[:m].tolist() == idx and kind[:m].tolist() == kd, c.name
    assert group_off[:groups + 1].tolist() == go, c.name
    assert (out[total:] == GUARD8).all() and (out_off[m + 1:] == GUARD64).all() and (doc_idx[m:] == GUARD64).all(), c.name
    assert (kind[m:] == GUARD8).all() and (group_off[groups + 1:] == GUARD64).all(), c.name
    raw = out.base                                   # the allocation: nothing in front of the shifted output is touched either
    at = out.ctypes.data - raw.ctypes.data
    assert at >= shift and (raw[:at] == GUARD8).all() and (raw[at + out.size:] == GUARD8).all(), c.name


def test_fixed_cases():
    want = X.expected()
    for i, c in enumerate(X.fixed_cases()):
        check(c, want[c.name], (0, 1, 3, 8, 15)[i % 5])


def test_random_batches():
    want = X.expected()
    for i, c in enumerate(X.random_cases()):
        check(c, want[c.name], (0, 1, 3, 8, 15)[i % 5])


def test_without_reach_and_fence_it_is_the_select():
    for c in S.all_cases():
        m, total, out, out_off, doc_idx = select_docs_host(c.blob, c.doc_off, c.rows, c.n_cols, c.want, c.mode, c.also)
        km, hits, groups, kt, kout, koff, kidx, kind, group_off = context_docs_host(c.blob, c.doc_off, c.rows, c.n_cols, c.want, c.mode, c.also)
        assert (km, hits, kt) == (m, m, total), c.name
        assert kout.tobytes() == out.tobytes() and koff.tolist() == out_off.tolist() and kidx.tolist() == doc_idx.tolist(), c.name
        assert (kind == 1).all(), c.name
        idx = doc_idx.tolist()
        runs = [r for r in range(m) if r == 0 or idx[r - 1] != idx[r] - 1]                        # the maximal runs of selected documents
        assert group_off.tolist() == runs + [m] and groups == len(runs), c.name


def cap_case():
    return next(c for c in X.fixed_cases() if c.name == "65 documents, fences")


def test_cap_protocol():
    c = cap_case()
    data, off, idx, kd, go = X.expected()[c.name]
    total, m, g = len(data), len(idx), len(go) - 1
    assert m >= 4 and g >= 3 and 0 in kd and 1 in kd
    k3 = next(k for k in range(m) if off[k + 1] - off[k] >= 2)
    mid = off[k3] + 1                                    # inside a document
    args = (c.blob, c.doc_off, c.rows, c.n_cols, c.want, c.mode, c.also, c.before, c.after, c.fence)
    for shift in (0, 5):
        for cb in (total, total - 1, mid, 1, 0):
            for cd in (m, m - 1, 1, 0):
                for cg in (g, g - 1, 1, 0):
                    gm, gh, gg, gt, out, out_off, doc_idx, kind, group_off = context_docs_host(*args, cap_bytes=cb, cap_docs=cd, cap_groups=cg, guard=24,
                                                                                               out_shift=shift)
                    assert (gm, gh, gg, gt) == (m, sum(kd), g, total), (cb, cd, cg)
                    assert out[:cb].tobytes() == data[:cb] and (out[min(total, cb):] == GUARD8).all(), (cb, cd, cg)
                    k = min(m, cd)
                    assert out_off[:k + 1].tolist() == off[:k + 1] and (out_off[k + 1:] == GUARD64).all(), (cb, cd, cg)
                    assert doc_idx[:k].tolist() == idx[:k] and (doc_idx[k:] == GUARD64).all(), (cb, cd, cg)
                    assert kind[:k].tolist() == kd[:k] and (kind[k:] == GUARD8).all(), (cb, cd, cg)
                    j = min(g, cg)
                    assert group_off[:j + 1].tolist() == go[:j + 1] and (group_off[j + 1:] == GUARD64).all(), (cb, cd, cg)
    # count only: no arrays at all
    r = context_docs_host(*args, cap_bytes=0, cap_docs=0, cap_groups=0, count_only=True)
    assert r[:4] == (m, sum(kd), g, total)
    # no documents: entry 0 of both offset arrays alone
    r = context_docs_host(b"", [0], np.zeros((0, 1), np.uint32), 7, None, "any", None, 2, 2, cap_bytes=0, cap_docs=3, cap_groups=2, guard=2)
    assert r[:4] == (0, 0, 0, 0) and r[5][0] == 0 and (r[5][1:] == GUARD64).all() and r[8][0] == 0 and (r[8][1:] == GUARD64).all()
    # nothing selected: nothing written but the two leading entries
    c = next(c for c in X.fixed_cases() if c.name == "nothing selected")
    r = context_docs_host(c.blob, c.doc_off, c.rows, c.n_cols, c.want, c.mode, c.also, c.before, c.after, c.fence, cap_bytes=9, cap_docs=4,
                          cap_groups=4, guard=3)
    assert r[:4] == (0, 0, 0, 0) and (r[4] == GUARD8).all() and r[5][0] == 0 and (r[5][1:] == GUARD64).all()
    assert (r[6] == GUARD64).all() and (r[7] == GUARD8).all() and r[8][0] == 0 and (r[8][1:] == GUARD64).all()


def raw_call(L, blob, off, rows, n_cols, mode, also, fence, out, cb, oo, di, ki, cd, go, cg, want=None, before=1, after=1):
    cnt = [C.c_uint64(7) for _ in range(4)]
    p = lambda a: a.ctypes.data if a is not None else None   # noqa: E731
    rc = L.gft_debug_context_docs(p(blob), p(off), len(rows) if off is None else len(off) - 1, p(rows), n_cols, p(want), mode, p(also), before, after, p(fence), p(out), cb, p(oo),
                                  p(di), p(ki), cd, p(go), cg, *[C.byref(x) for x in cnt])
    return (rc,) + tuple(x.value for x in cnt)


def test_refusals():
    L = _lib.load()
    E = _lib.GFT_E_INVALID
    blob = np.arange(64, dtype=np.uint8)
    off = np.array([0, 10, 30, 64, 64], dtype=np.uint64)
    rows = np.array([[1], [0], [0], [0]], dtype=np.uint32)
    also, fence = np.zeros(4, dtype=np.uint8), np.zeros(4, dtype=np.uint8)
    out, oo, di, ki, go = np.zeros(64, np.uint8), np.zeros(5, np.uint64), np.zeros(4, np.uint64), np.zeros(4, np.uint8), np.zeros(3, np.uint64)

    def call(blob=blob, off=off, rows=rows, mode=0, also=also, fence=fence, out=out, cb=64, oo=oo, di=di, ki=ki, cd=4, go=go, cg=2):
        return raw_call(L, blob, off, rows, 1, mode, also, fence, out, cb, oo, di, ki, cd, go, cg)
    assert call() == (0, 2, 1, 1, 30)                                                                  # (kept, hits, groups, bytes)
    assert call(mode=3)[0] == E                                                                        # unknown mode
    assert call(out=None)[0] == E and call(oo=None)[0] == E and call(di=None)[0] == E                  # a cap without its array
    assert call(ki=None)[0] == E and call(go=None)[0] == E
    assert call(rows=None)[0] == E and call(off=None)[0] == E                                          # a null argument
    down = np.array([0, 30, 10, 64, 64], dtype=np.uint64)
    assert call(off=down)[0] == E                                                                      # offsets that descend
    huge = np.array([0, 10, 30, 30 + (1 << 32), 30 + (1 << 32)], dtype=np.uint64)
    assert call(off=huge, out=None, cb=0, oo=None, di=None, ki=None, cd=0, go=None, cg=0)[0] == E      # a document of 4 GiB (not kept)
    for name, target in (("text", blob), ("offsets", off), ("rows", rows), ("also", also), ("fence", fence)):
        view = np.frombuffer(target.data, dtype=np.uint8)
        assert call(out=view, cb=min(view.size, 3))[0] == E, name
        assert call(ki=view[:4])[0] == E, name
    big = np.zeros(256, dtype=np.uint8)
    assert call(out=big, oo=big[32:72].view(np.uint64))[0] == E                                        # two outputs
    assert call(out=big[128:], ki=big[0:4], go=big[0:24].view(np.uint64))[0] == E
    assert call(out=big[128:], di=big[0:32].view(np.uint64), go=big[16:40].view(np.uint64))[0] == E
    assert call() == (0, 2, 1, 1, 30)
    with pytest.raises(GftError):
        context_docs_host(blob, off, rows, 1, None, 5)
    with pytest.raises(ValueError):
        context_docs_host(blob, off, rows, 40, np.zeros(1, np.uint32))                                   # a mask of the wrong size


class NaiveEngine(SubstringEngine):
    """an injected substring engine: such a finder never takes the device route"""

    def BuildEngine(self, keywords, caseSensitive):
        self.keywords = list(keywords)

    def FindSubstrings(self, text):
        return [Match(text.find(k), k) for k in self.keywords if k in text]


LINES = [b"zero\n", b"ab\n", b"two\n", b"three\n", b"\n", b"five\n", b"xccd\n", b"seven\n", b"eight\n", b"nine\n", b"ab ccd\n", b"last"]
LINE_ROWS = [0, 1, 0, 0, 0, 0, 2, 0, 0, 0, 3, 0]                        # '"ab"' is expression 0, 'r"c+d"' expression 1


def host_route_finder():
    f = Finder(NaiveEngine(), PyRegexpEngine(), False, allow_no_device=True)
    f.AddExpressions(['"ab"', 'r"c+d"'])
    assert f._takes_device_route() is False
    return f


def test_context_lines_off_the_device_route_walk_on_the_host(monkeypatch):
    """what ContextLines does with the rows when the finder stays off the device route: the split and the context by the kernels'
    walk on the host.  ProcessTexts solves on the device whatever the engines are, so the rows are handed in here; the test below
    runs the same lines with the finder's own rows"""
    f = host_route_finder()

    def rows_of(blob=None, doc_off=None, **_):
        assert bytes(blob[:int(doc_off[-1])]) == b"".join(LINES) and doc_off.tolist() == np.cumsum([0] + [len(x) for x in LINES]).tolist()
        return np.array(LINE_ROWS, dtype=np.uint32).reshape(-1, 1)
    monkeypatch.setattr(f, "ProcessTexts", rows_of)
    check_context_lines(f, np.array(LINE_ROWS, dtype=np.uint32).reshape(-1, 1))
    f.close()


@pytest.mark.gpu
def test_context_lines_on_the_host_route():
    """a finder with a regex term decides on the host: rows from ProcessTexts (its solver runs on the device: the one test of this
    file that needs one), the context by the kernels' walk"""
    f = host_route_finder()
    rows = f.ProcessTexts(LINES)
    assert rows[:, 0].tolist() == LINE_ROWS
    check_context_lines(f, rows)
    got = f.ContextLines(b"", 3, 3)
    assert got[0] == b"" and got[1].tolist() == [0] and got[2].size == 0 and got[3].size == 0 and got[4].tolist() == [0]
    f.close()


def check_context_lines(f, rows):
    lines = LINES
    blob = b"".join(lines)
    off = np.concatenate([[0], np.cumsum([len(x) for x in lines])]).astype(np.uint64)
    for before, after, want, mode in ((0, 0, None, "any"), (1, 1, None, "any"), (2, 0, f.want_mask(indices=[1]), "any"), (0, 3, None, "all"),
                                      (1, 0, f.want_mask(indices=[0]), "none"), (X.U64, 0, f.want_mask(indices=[1]), "any")):
        data, out_off, idx, kind, go = X.reference(blob, off, rows, 2, want, mode, None, before, after, None)
        got = f.ContextLines(blob, before, after, want, mode)
        assert got[0] == data and got[1].tolist() == out_off and got[2].tolist() == idx and got[3].tolist() == kind and got[4].tolist() == go, (before, after, mode)
    got = f.ContextLines(blob, 1, 1)
    assert got[2].tolist() == [0, 1, 2, 5, 6, 7, 9, 10, 11] and got[3].tolist() == [0, 1, 0, 0, 1, 0, 0, 1, 0] and got[4].tolist() == [0, 3, 6, 9]
