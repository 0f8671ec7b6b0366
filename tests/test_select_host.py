"""The documents that matched, gathered into one blob -- the host half: gft_debug_select_docs -- the kernels' walk
(csrc/gft_select_piece.hpp) tile by tile on the host -- against the reference of select_docs.py on every fixed and random case, the
cap protocol with guard patterns behind both caps, the refusals, the two masks of the callers.  No GPU needed."""
import ctypes as C
import re
import os

import numpy as np
import pytest

import select_docs as S
from gofindthem_amd import _lib, group
from gofindthem_amd.engine import GftError, select_docs_host, select_shape
from gofindthem_amd.finder import Finder, Match, SubstringEngine

GUARD8, GUARD64 = 0xA5, 0xA5A5A5A5A5A5A5A5
NAMES = ("gft_select_docs_device", "gft_debug_select_docs", "gft_debug_select_shape", "gft_finder_select_docs_device")


def test_symbols_and_shape():
    L = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gft.h")).read()
    for name in NAMES:
        assert hasattr(L, name) and name in _lib.SYMBOLS
        assert re.search(r"\b%s\(" % name, header)
    for word in ("GFT_SELECT_ANY = 0", "GFT_SELECT_ALL = 1", "GFT_SELECT_NONE = 2"):
        assert word in header
    chunk, trip, tile = select_shape()
    assert chunk == 16 and trip == 64 * chunk and tile % trip == 0 and tile >= trip


def test_the_reference_on_the_contract_examples():
    """the reference itself, on cases small enough to read: columns 0..2, documents ab, c, (empty), def"""
    off = [0, 2, 3, 3, 6]
    rows = np.array([[0b001], [0b110], [0b000], [0b111]], dtype=np.uint32) | np.uint32(0xFFFFFFF8)       # (tail bits: ones)
    want = np.array([0b011 | 0xFFFFFFF8], dtype=np.uint32)
    assert S.reference(b"abcdef", off, rows, 3, want, "any", None) == (b"abcdef", [0, 2, 3, 6], [0, 1, 3])
    assert S.reference(b"abcdef", off, rows, 3, want, "all", None) == (b"def", [0, 3], [3])
    assert S.reference(b"abcdef", off, rows, 3, want, "none", None) == (b"", [0, 0], [2])
    assert S.reference(b"abcdef", off, rows, 3, None, "all", None) == (b"def", [0, 3], [3])
    assert S.reference(b"abcdef", off, rows, 3, np.array([0xFFFFFFF8], dtype=np.uint32), "all", None)[2] == [0, 1, 2, 3]
    assert S.reference(b"abcdef", off, rows, 3, want, "all", [0, 1, 0, 0]) == (b"cdef", [0, 1, 4], [1, 3])
    assert S.reference(b"abcdef", off, rows[:, :0], 0, None, "any", None)[2] == [] and S.reference(b"abcdef", off, rows[:, :0], 0, None, "none", None)[2] == [0, 1, 2, 3]
    S.assert_not_vacuous()


def check(c, want_result, shift=0):
    m, total, out, out_off, doc_idx = select_docs_host(c.blob, c.doc_off, c.rows, c.n_cols, c.want, c.mode, c.also, guard=16, out_shift=shift)
    data, off, idx = want_result
    assert (m, total) == (len(idx), len(data)), c.name
    assert out[:total].tobytes() == data, c.name
    assert out_off[:m + 1].tolist() == off and doc_idx[:m].tolist() == idx, c.name
    assert (out[total:] == GUARD8).all() and (out_off[m + 1:] == GUARD64).all() and (doc_idx[m:] == GUARD64).all(), c.name
    raw = out.base                                   # the allocation: nothing in front of the shifted output is touched either
    at = out.ctypes.data - raw.ctypes.data
    assert at >= shift and (raw[:at] == GUARD8).all() and (raw[at + out.size:] == GUARD8).all(), c.name


def test_fixed_cases():
    want = S.expected()
    for c in S.fixed_cases():
        for shift in (0, 1, 3, 8, 15):
            check(c, want[c.name], shift)


def test_random_batches():
    want = S.expected()
    assert len(S.random_cases()) == 9 and max(len(c.doc_off) for c in S.random_cases()) == 5001
    for i, c in enumerate(S.random_cases()):
        check(c, want[c.name], (0, 1, 3, 8, 15)[i % 5])


def test_all_with_an_empty_mask_and_none_as_the_complement_of_any():
    for c in S.all_cases():
        n = len(c.doc_off) - 1
        W = (c.n_cols + 31) // 32
        empty = np.zeros(W, dtype=np.uint32)
        if c.n_cols & 31:
            empty[W - 1] = (0xFFFFFFFF << (c.n_cols & 31)) & 0xFFFFFFFF                                     # (tail bits: ones)
        m, _, _, _, idx = select_docs_host(c.blob, c.doc_off, c.rows, c.n_cols, empty, "all")
        assert m == n and idx[:m].tolist() == list(range(n)), c.name
        a = select_docs_host(c.blob, c.doc_off, c.rows, c.n_cols, c.want, "any")
        b = select_docs_host(c.blob, c.doc_off, c.rows, c.n_cols, c.want, "none")
        ia, ib = a[4][:a[0]].tolist(), b[4][:b[0]].tolist()
        assert sorted(ia + ib) == list(range(n)) and not set(ia) & set(ib), c.name
        assert a[1] + b[1] == int(c.doc_off[n] - c.doc_off[0]), c.name


def cap_case():
    return next(c for c in S.fixed_cases() if c.name == "edge lengths, every other one")


def caps_of(data, off, idx):
    total, m = len(data), len(idx)
    mid = (off[3] + off[4]) // 2                     # inside a document
    assert off[3] < mid < off[4]
    return [total, total - 1, mid, 1, 0], [m, m - 1, 1, 0]


def test_cap_protocol():
    c = cap_case()
    data, off, idx = S.expected()[c.name]
    total, m = len(data), len(idx)
    cbs, cds = caps_of(data, off, idx)
    for shift in (0, 5):
        for cb in cbs:
            for cd in cds:
                gm, gt, out, out_off, doc_idx = select_docs_host(c.blob, c.doc_off, c.rows, c.n_cols, c.want, c.mode, c.also, cap_bytes=cb, cap_docs=cd,
                                                                 guard=24, out_shift=shift)
                assert (gm, gt) == (m, total), (cb, cd)
                assert out[:cb].tobytes() == data[:cb] and (out[min(total, cb):] == GUARD8).all(), (cb, cd)
                k = min(m, cd)
                assert out_off[:k + 1].tolist() == off[:k + 1] and (out_off[k + 1:] == GUARD64).all(), (cb, cd)
                assert doc_idx[:k].tolist() == idx[:k] and (doc_idx[k:] == GUARD64).all(), (cb, cd)
    # count only: no arrays at all
    gm, gt, _, _, _ = select_docs_host(c.blob, c.doc_off, c.rows, c.n_cols, c.want, c.mode, c.also, cap_bytes=0, cap_docs=0, count_only=True)
    assert (gm, gt) == (m, total)
    # no documents: entry 0 alone
    gm, gt, _, out_off, _ = select_docs_host(b"", [0], np.zeros((0, 1), np.uint32), 7, None, "any", cap_bytes=0, cap_docs=3, guard=2)
    assert (gm, gt) == (0, 0) and out_off[0] == 0 and (out_off[1:] == GUARD64).all()


def raw_call(L, blob, off, rows, n_cols, mode, also, out, cb, oo, di, cd, want=None):
    m, t = C.c_uint64(7), C.c_uint64(7)
    p = lambda a: a.ctypes.data if a is not None else None   # noqa: E731
    rc = L.gft_debug_select_docs(p(blob), p(off), len(off) - 1, p(rows), n_cols, p(want), mode, p(also), p(out), cb, p(oo), p(di), cd, C.byref(m),
                                 C.byref(t))
    return rc, m.value, t.value


def test_refusals():
    L = _lib.load()
    E = _lib.GFT_E_INVALID
    blob = np.arange(64, dtype=np.uint8)
    off = np.array([0, 10, 30, 64], dtype=np.uint64)
    rows = np.array([[1], [0], [1]], dtype=np.uint32)
    also = np.zeros(3, dtype=np.uint8)
    out, oo, di = np.zeros(64, np.uint8), np.zeros(4, np.uint64), np.zeros(3, np.uint64)
    ok = lambda: raw_call(L, blob, off, rows, 1, 0, also, out, 64, oo, di, 3)   # noqa: E731
    assert ok() == (0, 2, 44)
    assert raw_call(L, blob, off, rows, 1, 3, also, out, 64, oo, di, 3)[0] == E                       # unknown mode
    assert raw_call(L, blob, off, rows, 1, 0, also, None, 64, oo, di, 3)[0] == E                      # a cap without its array
    assert raw_call(L, blob, off, rows, 1, 0, also, out, 64, None, di, 3)[0] == E
    assert raw_call(L, blob, off, rows, 1, 0, also, out, 64, oo, None, 3)[0] == E
    assert raw_call(L, blob, off, None, 1, 0, also, out, 64, oo, di, 3)[0] == E                       # columns but no rows
    down = np.array([0, 30, 10, 64], dtype=np.uint64)
    assert raw_call(L, blob, down, rows, 1, 0, also, out, 64, oo, di, 3)[0] == E                      # offsets that descend
    huge = np.array([0, 10, 10 + (1 << 32), 10 + (1 << 32)], dtype=np.uint64)
    assert raw_call(L, blob, huge, rows, 1, 0, also, None, 0, None, None, 0)[0] == E                  # a document of 4 GiB (not selected)
    big = np.zeros(256, dtype=np.uint8)
    for name, target in (("text", blob), ("offsets", off), ("rows", rows), ("also", also)):
        view = np.frombuffer(target.data, dtype=np.uint8)
        assert raw_call(L, blob, off, rows, 1, 0, also, view, min(view.size, 3), oo, di, 3)[0] == E, name
    assert raw_call(L, big[:64], off, rows, 1, 0, also, big[100:], 64, big[60:124].view(np.uint64)[:4], di, 3)[0] == E      # offsets over the text
    assert raw_call(L, blob, off, rows, 1, 0, also, big, 64, big[32:64].view(np.uint64), di, 3)[0] == E                        # two outputs
    assert ok() == (0, 2, 44)
    with pytest.raises(GftError):
        select_docs_host(blob, off, rows, 1, None, 5)
    with pytest.raises(ValueError):
        select_docs_host(blob, off, rows, 40, np.zeros(1, np.uint32))                                   # a mask of the wrong size


def test_the_text_in_front_of_document_zero_is_not_needed():
    """only blob[doc_off[0], doc_off[n]) is read: a NULL blob is fine when nothing of it is selected or it is empty"""
    L = _lib.load()
    off = np.array([5, 5, 5], dtype=np.uint64)
    rows = np.array([[1], [1]], dtype=np.uint32)
    oo, di = np.zeros(3, np.uint64), np.zeros(2, np.uint64)
    assert raw_call(L, None, off, rows, 1, 0, None, None, 0, oo, di, 2) == (0, 2, 0)
    assert oo.tolist() == [0, 0, 0] and di.tolist() == [0, 1]


def test_want_mask():
    f = Finder(None, None, False, allow_no_device=True)
    for i in range(40):
        f.AddExpressionWithTag('"w%d"' % i, "odd" if i % 2 else "even" if i % 4 else "four")
    assert f.want_mask().tolist() == [0xFFFFFFFF, 0xFF]
    assert f.want_mask(indices=[0, 31, 32, 39]).tolist() == [0x80000001, 0x81]
    assert f.want_mask(tags=["odd"]).tolist() == [0xAAAAAAAA, 0xAA]
    assert f.want_mask(tags="four").tolist() == [0x11111111, 0x11]
    assert f.want_mask(indices=[1], tags=["four", "even"]).tolist() == [0x55555557, 0x55]
    assert f.want_mask(indices=[]).tolist() == [0, 0]
    with pytest.raises(ValueError):
        f.want_mask(tags=["no such tag"])
    with pytest.raises(ValueError):
        f.want_mask(indices=[40])


def test_rule_mask():
    f = Finder(None, None, False, allow_no_device=True)
    f.AddExpressionWithTag('"alpha"', "t1")
    f.AddExpressionWithTag('"beta"', "t2")
    g = group.NewFinderWithRules(f, {"ab": ['"t1" and "t2"', '"t1" or "t2"'], "only a": ['"t1" and not "t2"'], "none": ['not "t1"']})
    names = [r for r, _ in g.rule_exprs()]
    assert sorted(names) == ["ab", "ab", "none", "only a"]
    bit = lambda rule: sum(1 << i for i, r in enumerate(names) if r == rule)   # noqa: E731
    assert g.rule_mask().tolist() == [0xF]
    assert g.rule_mask(["ab"]).tolist() == [bit("ab")] and bin(bit("ab")).count("1") == 2
    assert g.rule_mask("none").tolist() == [bit("none")]
    assert g.rule_mask(["none", "only a"]).tolist() == [bit("none") | bit("only a")]
    assert g.rule_mask([]).tolist() == [0]
    with pytest.raises(ValueError):
        g.rule_mask(["no such rule"])


class NaiveEngine(SubstringEngine):
    """an injected substring engine: such a finder never takes the device route"""

    def BuildEngine(self, keywords, caseSensitive):
        self.keywords = list(keywords)

    def FindSubstrings(self, text):
        return [Match(text.find(k), k) for k in self.keywords if k in text]


def test_select_lines_asks_the_handle_for_its_route():
    import torch
    f = Finder(None, None, False, allow_no_device=True)
    f.AddExpression('"ab"')
    assert f._takes_device_route() == torch.cuda.is_available()          # (without a device: the host walk, not a failed upload)
    g = Finder(NaiveEngine(), None, False, allow_no_device=True)
    g.AddExpression('"ab"')
    assert g._takes_device_route() is False
