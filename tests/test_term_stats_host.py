"""Term statistics and column counts on the host: gft_debug_term_stats and gft_debug_count_columns -- the kernels' walks workgroup by
workgroup, step by step and lane by lane through the header the kernels compile -- against the numpy reference of term_stats.py on
the fixed cases at the walk's borders (from gft_debug_stats_shape), the accumulation, the 64-bit carry, every output NULL on its
own, the refusals, which must leave every output byte for byte, the overlaps, and seeded Zipf lists.  All comparisons are exact; no
device needed."""
import ctypes as C

import numpy as np
import pytest

import term_stats as TS
from gofindthem_amd import _lib
from gofindthem_amd.engine import Engine, GftError, count_columns_host, stats_shape, term_stats_host

NAMES = ("gft_term_stats_device", "gft_count_columns_device", "gft_batch_term_stats_device", "gft_debug_term_stats", "gft_debug_count_columns",
         "gft_debug_stats_shape", "gft_finder_term_stats_device")
SH = stats_shape()
FIXED = TS.fixed_cases(SH)
RANDOM = TS.random_cases(SH, 36)
COLUMNS = TS.column_cases(SH)


def run(off, term, n_docs, n_terms, flags, doc_base, occ, docs, first):
    try:
        term_stats_host(off if off is not None else np.zeros(0, np.uint64), term, n_terms, occ, docs, first, flags, doc_base, n_docs=n_docs)
    except GftError as e:
        return e.code
    return 0


def run_cols(bm, n_rows, n_cols, row_idx, flags, count):
    try:
        count_columns_host(bm, n_rows, n_cols, count, row_idx, flags)
    except GftError as e:
        return e.code
    return 0


def test_symbols_present():
    L = _lib.load()
    header = open(_lib.__file__.replace("gofindthem_amd/_lib.py", "include/gft.h")).read()
    for name in NAMES:
        assert hasattr(L, name) and name in _lib.SYMBOLS and name in header
    assert "GFT_STATS_ACCUMULATE 1u" in header and _lib.GFT_STATS_ACCUMULATE == TS.ACC
    assert SH["large_entries"] == SH["step_entries"] + 1 and SH["set_slots"] >= 2 * SH["step_entries"]
    assert SH["bitset_lds_terms"] >= 100000                        # (the dictionary of the headline batch keeps its bitset in LDS)


@pytest.mark.parametrize("case", FIXED, ids=[c.name for c in FIXED])
def test_fixed(case):
    TS.check_case(run, case)
    TS.check_case(run, case, doc_base=(1 << 40) + 3)


@pytest.mark.parametrize("case", RANDOM, ids=[c.name for c in RANDOM])
def test_random(case):
    TS.check_case(run, case, doc_base=12345)


def test_null_outputs():
    for case in FIXED[:3] + RANDOM[:2]:
        TS.check_null_outputs(run, case)


@pytest.mark.parametrize("name", ["step_sum_%d" % SH["step_entries"], "ranges", "large_between_small", "cut_middle", "set_collide"])
def test_accumulate_halves(name):
    case = next(c for c in FIXED if c.name == name)
    for cut in sorted({0, 1, case.n_docs // 2, case.n_docs - 1, case.n_docs}):
        TS.check_accumulate_halves(run, case, cut)


def test_accumulate_carry():
    TS.check_accumulate_carry(run)


REFUSALS = TS.refusal_inputs(SH)


@pytest.mark.parametrize("r", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(r):
    TS.check_refusal(run, *r[1:])


def test_overlaps():
    """an output that overlaps an input or another output: refused, nothing written"""
    L = _lib.load()
    case = next(c for c in FIXED if c.name == "off0")
    nt = case.n_terms
    pool = np.full(4 * nt + 8, 0x77, np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)                      # noqa: E731
    views = {"same": (pool[:nt], pool[:nt], pool[2 * nt:3 * nt]), "shifted": (pool[:nt], pool[nt:2 * nt], pool[2 * nt - 1:3 * nt - 1]),
             "occ_first": (pool[:nt], pool[2 * nt:3 * nt], pool[nt - 1:2 * nt - 1])}
    for name, (a, b, c) in views.items():
        keep = pool.copy()
        assert L.gft_debug_term_stats(p(case.off), p(case.term), case.n_docs, nt, 0, 0, p(a), p(b), p(c)) == TS.E_INVALID, name
        assert (pool == keep).all()
    # an output over the offsets, over the entries (uint64 views of the inputs' own memory)
    case = next(c for c in FIXED if c.name == "cut_middle")
    nt = case.n_terms
    off, term = case.off.copy(), case.term.copy()
    for name, out in (("offsets", off[3:3 + nt]), ("entries", term[778:778 + 2 * nt].view(np.uint64))):
        keep_o, keep_t = off.copy(), term.copy()
        assert L.gft_debug_term_stats(p(off), p(term), case.n_docs, nt, 0, 0, None, p(out), None) == TS.E_INVALID, name
        assert (off == keep_o).all() and (term == keep_t).all()
    # (the garbage in front of off[0] is no input: an output there is fine)
    assert L.gft_debug_term_stats(p(off), p(term), case.n_docs, nt, 0, 0, p(term[:2 * nt].view(np.uint64)), None, None) == 0
    # the column counts over the bitmap
    bm = np.full((8, 2), 0xFFFFFFFF, np.uint32)
    keep = bm.copy()
    assert L.gft_debug_count_columns(p(bm), 8, 40, None, 0, p(bm.view(np.uint64))) == TS.E_INVALID and (bm == keep).all()
    idx = np.arange(40, dtype=np.uint64) % 8
    assert L.gft_debug_count_columns(p(bm), 40, 40, p(idx), 0, p(idx)) == TS.E_INVALID and (idx == np.arange(40) % 8).all()


@pytest.mark.parametrize("c", COLUMNS, ids=[c[0] for c in COLUMNS])
def test_columns(c):
    TS.check_columns(run_cols, *c)


def test_engine_wrappers():
    case = FIXED[0]
    body = case.term
    got = Engine.term_stats_host(case.off, body, case.n_terms)
    for g, w in zip(got, TS.reference(case.off, body, case.n_docs, case.n_terms)):
        assert (g == w).all()
    again = Engine.term_stats_host(case.off, body, case.n_terms, accumulate_into=got, doc_base=50)
    assert (again[0] == 2 * TS.reference(case.off, body, case.n_docs, case.n_terms)[0]).all()
    name, bm, n_cols, idx = COLUMNS[-4]
    assert (Engine.count_columns_host(bm, n_cols, idx) == TS.columns_reference(bm, n_cols, idx)).all()
    assert Engine.stats_shape() == SH
