"""Sparse batch results on the host: gft_debug_compact_host (the restatement of the device compaction, and the code the
finder runs for a bitmap that was completed on the host) against numpy, and the finder's tag numbering.  No device."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden
from gofindthem_amd import _lib
from gofindthem_amd.engine import compact_host
from gofindthem_amd.finder import Finder

N_EXPRS = [1, 31, 32, 33, 64, 1000, 2049, 5000]
N_DOCS = [0, 1, 63, 64, 65, 1000]
DENSITY = [0.0, 0.01, 0.5, 1.0]


def make_bitmap(n_docs, n_exprs, density, seed, junk=True):
    """-> (bitmap [n_docs, W] uint32, bits [n_docs, n_exprs] bool).  junk: the padding bits of the last word are random"""
    rng = np.random.default_rng(seed)
    words = (n_exprs + 31) // 32
    bits = rng.random((n_docs, n_exprs)) < density if 0 < density < 1 else np.full((n_docs, n_exprs), density >= 1)
    full = np.zeros((n_docs, words * 32), dtype=np.uint8)
    full[:, :n_exprs] = bits
    if junk:
        full[:, n_exprs:] = rng.integers(0, 2, size=(n_docs, words * 32 - n_exprs))
    bm = np.ascontiguousarray(np.packbits(full, axis=1, bitorder="little")).view(np.uint32).reshape(n_docs, words)
    return bm, bits


def numpy_csr(bm, n_exprs, labels=None):
    """the restatement: unpack the row bytes, truncate to n_exprs, list the set bits row by row"""
    n_docs = bm.shape[0]
    bits = np.unpackbits(np.ascontiguousarray(bm).view(np.uint8).reshape(n_docs, bm.shape[1] * 4), axis=1, bitorder="little")[:, :n_exprs]
    row_off = np.zeros(n_docs + 1, dtype=np.uint64)
    row_off[1:] = np.cumsum(bits.sum(axis=1, dtype=np.uint64), dtype=np.uint64)
    expr_idx = np.nonzero(bits)[1].astype(np.uint32)          # (row-major: document order, ascending inside a document)
    return row_off, expr_idx, (np.asarray(labels, np.uint32)[expr_idx] if labels is not None else None)


def make_labels(n_exprs, seed=5):
    return np.random.default_rng(seed).integers(0, 2 ** 32, size=n_exprs, dtype=np.uint64).astype(np.uint32)


@pytest.mark.parametrize("density", DENSITY)
@pytest.mark.parametrize("n_docs", N_DOCS)
@pytest.mark.parametrize("n_exprs", N_EXPRS)
def test_compact_host_equals_numpy(n_exprs, n_docs, density):
    bm, bits = make_bitmap(n_docs, n_exprs, density, seed=n_exprs * 7919 + n_docs)
    labels = make_labels(n_exprs)
    want = numpy_csr(bm, n_exprs, labels)
    assert int(want[0][-1]) == int(bits.sum())                 # (the padding junk is not counted)
    ro, ei, lb, total = compact_host(bm, n_exprs, labels)
    assert total == int(want[0][-1])
    assert np.array_equal(ro, want[0]) and np.array_equal(ei, want[1]) and np.array_equal(lb, want[2])
    # without labels: the same lists
    ro2, ei2, lb2, total2 = compact_host(bm, n_exprs)
    assert lb2 is None and total2 == total and np.array_equal(ro2, want[0]) and np.array_equal(ei2, want[1])


@pytest.mark.parametrize("n_exprs,n_docs", [(33, 65), (1000, 1000), (2049, 64)])
def test_cap_below_total_writes_a_prefix_and_nothing_behind_it(n_exprs, n_docs):
    L = _lib.load()
    bm, _ = make_bitmap(n_docs, n_exprs, 0.5, seed=11)
    labels = make_labels(n_exprs)
    want = numpy_csr(bm, n_exprs, labels)
    total = int(want[0][-1])
    for cap in (0, 1, total // 3, total - 1, total, total + 5):
        canary = 0xDEADBEEF
        ei = np.full(total + 64, canary, dtype=np.uint32)
        lb = np.full(total + 64, canary, dtype=np.uint32)
        ro = np.zeros(n_docs + 1, dtype=np.uint64)
        t = C.c_uint64()
        rc = L.gft_debug_compact_host(bm.ctypes.data, n_docs, n_exprs, labels.ctypes.data, ro.ctypes.data, ei.ctypes.data,
                                      lb.ctypes.data, cap, C.byref(t))
        assert rc == 0 and t.value == total
        assert np.array_equal(ro, want[0])                     # complete whatever cap is
        n = min(cap, total)
        assert np.array_equal(ei[:n], want[1][:n]) and np.array_equal(lb[:n], want[2][:n])
        assert (ei[n:] == canary).all() and (lb[n:] == canary).all()


def test_compact_host_rejects_missing_buffers():
    L = _lib.load()
    bm, _ = make_bitmap(4, 40, 0.5, seed=1)
    ro = np.zeros(5, dtype=np.uint64)
    ei = np.zeros(200, dtype=np.uint32)
    assert L.gft_debug_compact_host(bm.ctypes.data, 4, 40, None, None, ei.ctypes.data, None, 200, None) == _lib.GFT_E_INVALID
    assert L.gft_debug_compact_host(bm.ctypes.data, 4, 40, None, ro.ctypes.data, None, None, 200, None) == _lib.GFT_E_INVALID
    assert L.gft_debug_compact_host(bm.ctypes.data, 4, 40, None, ro.ctypes.data, ei.ctypes.data, ei.ctypes.data, 200, None) == _lib.GFT_E_INVALID
    assert L.gft_debug_compact_host(bm.ctypes.data, 4, 40, None, ro.ctypes.data, ei.ctypes.data, None, 200, None) == 0   # total may be NULL


# ---- tags ------------------------------------------------------------------------------------------------------------
def test_tag_ids_are_numbered_by_first_appearance():
    f = Finder(caseSensitive=True, allow_no_device=True)
    assert f.tags() == [] and f.expression_tag_id(0) == -1
    f.AddExpression('"a"')                                     # the empty tag is a tag like any other
    f.AddExpressionsWithTag(['"b"', '"c" and "d"'], "t1")
    f.AddExpressionsWithTag(['"e"'], "")
    f.AddExpressionsWithTag(['"f"', '"g"'], "t2")
    f.AddExpressionWithTag('"h"', "t1")
    f.AddExpression('"i"')
    assert f.tags() == ["", "t1", "t2"]
    assert [f.expression_tag_id(i) for i in range(f.n_expressions)] == [0, 1, 1, 0, 2, 2, 1, 0]
    assert f.expression_tag_id(f.n_expressions) == -1
    assert [f.tags()[f.expression_tag_id(i)] for i in range(f.n_expressions)] == [f.expression(i, tree=False)[1] for i in range(f.n_expressions)]
    f.close()


def test_a_refused_expression_registers_no_tag():
    f = Finder(caseSensitive=True, allow_no_device=True)
    f.AddExpressionWithTag('"a"', "x")
    with pytest.raises(Exception):
        f.AddExpressionWithTag('"a" and', "never")
    assert f.tags() == ["x"] and f.n_expressions == 1
    f.close()


def test_tag_ids_of_the_reference_example():
    sec = load_golden("examples.json")["case_sensitive"]
    assert [t for _, t in sec["expressions"]] == ["test", "test2", "test", "", ""]
    f = Finder(caseSensitive=True, allow_no_device=True)
    for e, tag in sec["expressions"]:
        f.AddExpressionWithTag(e, tag)
    assert f.tags() == ["test", "test2", ""]
    assert [f.expression_tag_id(i) for i in range(5)] == [0, 1, 0, 2, 2]
    L = _lib.load()
    assert L.gft_finder_n_tags(f._h) == 3
    p, n = C.c_void_p(), C.c_uint32()
    assert L.gft_finder_tag(f._h, 3, C.byref(p), C.byref(n)) == _lib.GFT_E_INVALID
    assert L.gft_finder_tag(f._h, 1, C.byref(p), C.byref(n)) == 0 and C.string_at(p, n.value) == b"test2"
    f.close()

