"""Documents routed to per-bucket runs of one blob -- the host half: gft_debug_route_docs -- the kernels' walk
(csrc/gft_route_piece.hpp, and the select's copy walk) tile by tile on the host -- against the reference of route_docs.py on every
fixed case and on 200 seeded random batches, the cap protocol with guard patterns behind both caps, the refusals, the masks of the
callers.  No GPU needed."""
import os
import re

import numpy as np
import pytest

import route_docs as R
from gofindthem_amd import _lib
from gofindthem_amd.engine import GftError, route_docs_host, route_shape
from gofindthem_amd.finder import Finder

GUARD8, GUARD64 = 0xA5, 0xA5A5A5A5A5A5A5A5
NAMES = ("gft_route_docs_device", "gft_debug_route_docs", "gft_debug_route_shape", "gft_finder_route_docs_device")


def test_symbols_and_shape():
    L = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gft.h")).read()
    for name in NAMES:
        assert hasattr(L, name) and name in _lib.SYMBOLS
        assert re.search(r"\b%s\(" % name, header)
    for word in ("GFT_ROUTE_FIRST = 0", "GFT_ROUTE_EVERY = 1", "#define GFT_ROUTE_REST 1u", "#define GFT_ROUTE_MAX_BUCKETS 64"):
        assert word in header
    assert route_shape() >= 64 and route_shape() % 64 == 0


def test_the_reference_on_the_contract_examples():
    """the reference itself, on cases small enough to read: columns 0..2, documents ab, c, (empty), def"""
    off = [0, 2, 3, 3, 6]
    rows = np.array([[0b001], [0b110], [0b000], [0b111]], dtype=np.uint32) | np.uint32(0xFFFFFFF8)       # (tail bits: ones)
    masks = np.array([[0b100], [0b011]], dtype=np.uint32) | np.uint32(0xFFFFFFF8)
    assert R.reference(b"abcdef", off, rows, 3, masks, "every", False, None) == (b"cdefabcdef", [0, 1, 4, 6, 7, 10], [1, 3, 0, 1, 3], [0, 2, 5], [0, 4, 10])
    assert R.reference(b"abcdef", off, rows, 3, masks, "first", False, None) == (b"cdefab", [0, 1, 4, 6], [1, 3, 0], [0, 2, 3], [0, 4, 6])
    assert R.reference(b"abcdef", off, rows, 3, masks, "first", True, None) == (b"cdefab", [0, 1, 4, 6, 6], [1, 3, 0, 2], [0, 2, 3, 4], [0, 4, 6, 6])
    assert R.reference(b"abcdef", off, rows, 3, masks, "every", True, [0, 0, 0, 9]) == (b"cabcdef", [0, 1, 3, 4, 4, 7], [1, 0, 1, 2, 3], [0, 1, 3, 5], [0, 1, 4, 7])
    assert R.reference(b"abcdef", off, rows[:, :0], 0, masks[:, :0], "every", True, None)[2:] == ([0, 1, 2, 3], [0, 0, 0, 4], [0, 0, 0, 6])
    assert R.reference(b"abcdef", off, rows, 3, masks[:0], "every", False, None) == (b"", [0], [], [0], [0])
    R.assert_not_vacuous()


def check(c, want, shift=0):
    bucket_doc, bucket_byte, out, out_off, doc_idx = route_docs_host(c.blob, c.doc_off, c.rows, c.n_cols, c.masks, c.mode, c.rest, c.also, guard=16,
                                                                     out_shift=shift)
    data, off, idx, bd, bb = want
    m, total = len(idx), len(data)
    assert bucket_doc.tolist() == bd and bucket_byte.tolist() == bb, c.name
    assert out[:total].tobytes() == data, c.name
    assert out_off[:m + 1].tolist() == off and doc_idx[:m].tolist() == idx, c.name
    assert (out[total:] == GUARD8).all() and (out_off[m + 1:] == GUARD64).all() and (doc_idx[m:] == GUARD64).all(), c.name
    raw = out.base                                   # the allocation: nothing in front of the shifted output is touched either
    at = out.ctypes.data - raw.ctypes.data
    assert at >= shift and (raw[:at] == GUARD8).all() and (raw[at + out.size:] == GUARD8).all(), c.name


def test_fixed_cases():
    want = R.expected()
    for c in R.fixed_cases():
        for shift in (0, 1, 8, 15):
            check(c, want[c.name], shift)


def test_random_batches():
    want = R.expected()
    assert len(R.random_cases()) == 200
    for i, c in enumerate(R.random_cases()):
        check(c, want[c.name], (0, 1, 3, 8, 15)[i % 5])


def test_no_documents():
    for rest in (False, True):
        bd, bb, _, out_off, _ = route_docs_host(b"", [0], np.zeros((0, 1), np.uint32), 7, np.ones((3, 1), np.uint32), "every", rest, cap_bytes=0,
                                                cap_docs=3, guard=2)
        assert bd.tolist() == [0] * (4 + rest) and bb.tolist() == [0] * (4 + rest) and out_off[0] == 0 and (out_off[1:] == GUARD64).all()


def test_cap_protocol():
    c = R.case("%d documents" % (2 * route_shape() + 1))
    data, off, idx, bd, bb = R.expected()[c.name]
    total, m = len(data), len(idx)
    assert bd[1] > 3 and bd[2] - bd[1] > 3 and bb[2] - bb[1] > 8
    in_bucket_1 = (bb[1] + bb[2]) // 2                 # inside bucket 1, and inside a document of it
    k = max(r for r in range(m) if off[r] <= in_bucket_1)
    if off[k] == in_bucket_1:
        in_bucket_1 += 1
    assert bb[1] < in_bucket_1 < bb[2] and off[k] < in_bucket_1 < off[k + 1]
    in_bucket_0 = bd[1] // 2
    assert 0 < in_bucket_0 < bd[1]
    for shift in (0, 5):
        for cb in (total, total - 1, in_bucket_1, 1, 0):
            for cd in (m, m - 1, in_bucket_0, 1, 0):
                gd, gb, out, out_off, doc_idx = route_docs_host(c.blob, c.doc_off, c.rows, c.n_cols, c.masks, c.mode, c.rest, c.also, cap_bytes=cb,
                                                                cap_docs=cd, guard=24, out_shift=shift)
                assert gd.tolist() == bd and gb.tolist() == bb, (cb, cd)
                assert out[:cb].tobytes() == data[:cb] and (out[min(total, cb):] == GUARD8).all(), (cb, cd)
                k = min(m, cd)
                assert out_off[:k + 1].tolist() == off[:k + 1] and (out_off[k + 1:] == GUARD64).all(), (cb, cd)
                assert doc_idx[:k].tolist() == idx[:k] and (doc_idx[k:] == GUARD64).all(), (cb, cd)
    # count only: no arrays at all
    gd, gb, _, _, _ = route_docs_host(c.blob, c.doc_off, c.rows, c.n_cols, c.masks, c.mode, c.rest, c.also, count_only=True)
    assert gd.tolist() == bd and gb.tolist() == bb
    # ... and no host arrays either: nothing to hand back, GFT_OK
    L = _lib.load()
    assert L.gft_debug_route_docs(c.blob.ctypes.data, c.doc_off.ctypes.data, len(c.doc_off) - 1, c.rows.ctypes.data, c.n_cols, c.masks.ctypes.data,
                                  len(c.masks), 1, 1, None, None, 0, None, None, 0, None, None) == 0


def raw_call(L, blob, off, rows, n_cols, masks, K, mode, flags, also, out, cb, oo, di, cd, bd="own", bb="own"):
    own_d, own_b = np.full(K + 2, 7, np.uint64), np.full(K + 2, 7, np.uint64)
    bd = own_d if isinstance(bd, str) else bd
    bb = own_b if isinstance(bb, str) else bb
    p = lambda a: a.ctypes.data if a is not None else None   # noqa: E731
    rc = L.gft_debug_route_docs(p(blob), p(off), len(off) - 1, p(rows), n_cols, p(masks), K, mode, flags, p(also), p(out), cb, p(oo), p(di), cd, p(bd), p(bb))
    return rc, own_d.tolist(), own_b.tolist()


def test_refusals():
    L = _lib.load()
    E, U = _lib.GFT_E_INVALID, _lib.GFT_E_UNSUPPORTED
    blob = np.arange(64, dtype=np.uint8)
    off = np.array([0, 10, 30, 64], dtype=np.uint64)
    rows = np.array([[1], [0], [3]], dtype=np.uint32)
    masks = np.array([[1], [2]], dtype=np.uint32)
    also = np.zeros(3, dtype=np.uint8)
    out, oo, di = np.zeros(128, np.uint8), np.zeros(5, np.uint64), np.zeros(4, np.uint64)
    ok = lambda: raw_call(L, blob, off, rows, 2, masks, 2, 1, 1, also, out, 128, oo, di, 4)   # noqa: E731
    assert ok() == (0, [0, 2, 3, 4], [0, 44, 78, 98])
    assert raw_call(L, blob, off, rows, 2, masks, 2, 2, 1, also, out, 128, oo, di, 4)[0] == E                    # unknown mode
    assert raw_call(L, blob, off, rows, 2, masks, 2, 1, 2, None, out, 128, oo, di, 4)[0] == E                    # unknown flag bits
    assert raw_call(L, blob, off, rows, 2, masks, 2, 1, 3, also, out, 128, oo, di, 4)[0] == E
    assert raw_call(L, blob, off, rows, 2, masks, 2, 1, 0, also, out, 128, oo, di, 4)[0] == E                    # also without rest
    assert raw_call(L, blob, off, rows, 2, masks, 2, 1, 0, None, out, 128, oo, di, 4)[0] == 0
    assert raw_call(L, blob, off, rows, 2, masks, 2, 1, 1, also, None, 128, oo, di, 4)[0] == E                   # a cap without its array
    assert raw_call(L, blob, off, rows, 2, masks, 2, 1, 1, also, out, 128, None, di, 4)[0] == E
    assert raw_call(L, blob, off, rows, 2, masks, 2, 1, 1, also, out, 128, oo, None, 4)[0] == E
    assert raw_call(L, blob, off, None, 2, masks, 2, 1, 1, also, out, 128, oo, di, 4)[0] == E                    # columns but no rows
    assert raw_call(L, blob, off, rows, 2, None, 2, 1, 1, also, out, 128, oo, di, 4)[0] == E                     # buckets but no masks
    many = np.ones((65, 1), dtype=np.uint32)
    wide = np.zeros(67, np.uint64)
    assert raw_call(L, blob, off, rows, 2, many, 65, 1, 0, None, None, 0, None, None, 0, wide, wide.copy())[0] == U     # 65 buckets
    assert raw_call(L, blob, off, rows, 2, many, 64, 1, 1, None, None, 0, None, None, 0, wide, wide.copy())[0] == U     # 64 and the rest
    assert raw_call(L, blob, off, rows, 2, many, 64, 1, 0, None, None, 0, None, None, 0, wide, wide.copy())[0] == 0
    assert raw_call(L, blob, off, rows, 2, many, 63, 1, 1, None, None, 0, None, None, 0, wide, wide.copy())[0] == 0
    down = np.array([0, 30, 10, 64], dtype=np.uint64)
    assert raw_call(L, blob, down, rows, 2, masks, 2, 1, 1, also, out, 128, oo, di, 4)[0] == E                   # offsets that descend
    huge = np.array([0, 10, 10 + (1 << 32), 10 + (1 << 32)], dtype=np.uint64)
    assert raw_call(L, blob, huge, rows, 2, masks, 2, 1, 0, None, None, 0, None, None, 0)[0] == E                # a document of 4 GiB (not routed)
    big = np.zeros(256, dtype=np.uint8)
    for name, target in (("text", blob), ("offsets", off), ("rows", rows), ("also", also), ("masks", masks)):
        view = np.frombuffer(target.data, dtype=np.uint8)
        assert raw_call(L, blob, off, rows, 2, masks, 2, 1, 1, also, view, min(view.size, 3), oo, di, 4)[0] == E, name
    assert raw_call(L, big[:64], off, rows, 2, masks, 2, 1, 1, also, big[128:], 128, big[56:96].view(np.uint64), di, 4)[0] == E     # offsets over the text
    assert raw_call(L, blob, off, rows, 2, masks, 2, 1, 1, also, big, 128, big[32:72].view(np.uint64), di, 4)[0] == E                # two outputs
    both = np.zeros(8, np.uint64)
    assert raw_call(L, blob, off, rows, 2, masks, 2, 1, 1, also, out, 128, oo, di, 4, both, both[2:])[0] == E                        # the two bucket arrays
    assert ok() == (0, [0, 2, 3, 4], [0, 44, 78, 98])
    with pytest.raises(GftError):
        route_docs_host(blob, off, rows, 2, masks, 5)
    with pytest.raises(ValueError):
        route_docs_host(blob, off, rows, 40, np.zeros((2, 1), np.uint32))                                        # masks of the wrong size


def test_the_text_in_front_of_document_zero_is_not_needed():
    """only blob[doc_off[0], doc_off[n]) is read: a NULL blob is fine when it is empty"""
    L = _lib.load()
    off = np.array([5, 5, 5], dtype=np.uint64)
    rows = np.array([[1], [1]], dtype=np.uint32)
    oo, di = np.zeros(3, np.uint64), np.zeros(2, np.uint64)
    rc, bd, bb = raw_call(L, None, off, rows, 1, np.array([[1]], np.uint32), 1, 1, 0, None, None, 0, oo, di, 2)
    assert (rc, bd[:2], bb[:2]) == (0, [0, 2], [0, 0])
    assert oo.tolist() == [0, 0, 0] and di.tolist() == [0, 1]


def test_route_masks():
    f = Finder(None, None, False, allow_no_device=True)
    for i in range(40):
        f.AddExpressionWithTag('"w%d"' % i, "odd" if i % 2 else "even" if i % 4 else "four")
    assert f.tags() == ["four", "odd", "even"]
    assert [m.tolist() for m in f.route_masks()] == [[0x11111111, 0x11], [0xAAAAAAAA, 0xAA], [0x44444444, 0x44]]
    got = f.route_masks(["odd", ["four", "even"], [0, 39], {"indices": [1], "tags": "four"}, []])
    assert [m.tolist() for m in got] == [[0xAAAAAAAA, 0xAA], [0x55555555, 0x55], [1, 0x80], [0x11111113, 0x11], [0, 0]]
    with pytest.raises(ValueError):
        f.route_masks(["no such tag"])
    with pytest.raises(ValueError) as e:
        f.route_masks([[0]] * 65)
    assert "64" in str(e.value)
    assert len(f.route_masks([[0]] * 64)) == 64
