"""The device INORD solver (csrc/gft_solve.hip: inord_group_wave, wide_expr_doc, inord_group_wide, and wave_succ_min under
all three) on random nested groups against the oracle, hit bitmap for hit bitmap.  The families -- seeds, trees, documents,
caller-supplied matches -- are those of inord_trees.py; test_inord_trees_host.py shows on the CPU that they are not vacuous
(both truth values, and documents in which the terms are present but not in order) and that the groups are narrow, wide or
beyond the device's limits as stated."""
import numpy as np
import pytest
import torch  # noqa: F401  (before libgft.so is loaded: both must share ONE HIP runtime, the one torch brings along)

import inord_trees as T
from oracle.pyoracle import POS_END, POS_START

pytestmark = pytest.mark.gpu

MODES = pytest.mark.parametrize("pos_mode", [POS_START, POS_END], ids=["start", "end"])   # (the `back` reach exists for START only)


@pytest.fixture(scope="module")
def eng():
    from gofindthem_amd.engine import Engine
    e = Engine()
    yield e
    e.close()


def run(eng, monkeypatch, fam, pos_mode, group_docs, counts=None):
    """the family's first n documents for every n of `counts` through gft_process -> the bitmap of the last count"""
    if group_docs is None:
        monkeypatch.delenv("GFT_SOLVE_GROUP_DOCS", raising=False)
    else:
        monkeypatch.setenv("GFT_SOLVE_GROUP_DOCS", group_docs)    # (read by gft_build and gft_set_programs)
    monkeypatch.delenv("GFT_SCAN_KERNEL", raising=False)
    eng.build(fam.terms, pos_end=(pos_mode == POS_END))
    assert eng.terms() == fam.terms
    eng.set_programs(fam.programs(), n_extra=len(fam.extra_lits))
    want = fam.reference(pos_mode)
    got = None
    for n in counts or [len(fam.texts)]:
        blob, off = fam.packed(n)
        got = eng.process(blob, off, extra=fam.extra_engine(n))
        if not np.array_equal(got, want[:n]):
            d, w = np.argwhere(got != want[:n])[0]
            i = int(w) * 32 + int(np.log2(int(got[d, w] ^ want[d, w]) & -int(got[d, w] ^ want[d, w])))
            raise AssertionError("%s, %d documents, group width %s, pos mode %d: document %d %r expression %d %s: oracle %d" % (
                fam.name, n, group_docs, pos_mode, d, fam.texts[d][:120], i, fam.exprs[i][:300], want[d, w] >> (i & 31) & 1))
    return got


def n_host_exprs(eng):
    from gofindthem_amd import _lib
    return _lib.load().gft_n_host_exprs(eng._h)


def check_named(fam, got, pos_mode):
    for e, d, at_start, at_end in fam.named:
        assert bool(got[d, e >> 5] >> (e & 31) & 1) is (at_end if pos_mode == POS_END else at_start), (fam.exprs[e], fam.texts[d], pos_mode)


@pytest.mark.parametrize("group_docs", [None, "32", "16", "8", "0"])
@MODES
def test_narrow_groups_over_short_documents(eng, monkeypatch, pos_mode, group_docs):
    """(a) a pair per lane, strided layout: ~150 random expressions over 1, 63, 64, 65 and 130 documents of 0-40 bytes at every
    group width, and the quirk rows of inord_trees.QUIRKS with the truth values derived by hand from the reference's
    dsl/expression.go:66-142 (solve) and :175-189 (getLowestIdxGTVal) as literals"""
    fam = T.family_narrow()
    got = run(eng, monkeypatch, fam, pos_mode, group_docs, [1, 63, 64, 65, 130])
    assert n_host_exprs(eng) == 0
    check_named(fam, got, pos_mode)


@pytest.mark.parametrize("group_docs", [None, "0"])
@MODES
def test_groups_at_the_limits(eng, monkeypatch, pos_mode, group_docs):
    """(b) 63 / 64 / 65 pairs alive, pair depth 32 / 33 / 64 / 65, 8 192 / 8 193 pairs alive, and a wide group under a
    boolean stack of more than 64 entries: the device answers what is within its limits, the host the three beyond"""
    fam = T.family_limits()
    run(eng, monkeypatch, fam, pos_mode, group_docs)
    assert n_host_exprs(eng) == sum(T.classify(w) == T.HOST for w in fam.programs()) == 3


@pytest.mark.parametrize("group_docs", [None, "8", "0"])
@MODES
def test_wide_groups_compacted(eng, monkeypatch, pos_mode, group_docs):
    """(c) groups of 70-400 leaves behind 0-130 ordinary words over documents that hold 0-12 of a group's terms: absent
    leaves are dropped, the pairs alive fit the lanes (wide_expr_doc); 1, 17, 64, 65 documents (documents are dealt to the
    sixteen waves of a workgroup)"""
    fam = T.family_wide()
    run(eng, monkeypatch, fam, pos_mode, group_docs, [1, 17, 64, 65])
    assert n_host_exprs(eng) == 0


@pytest.mark.parametrize("group_docs", [None, "8", "0"])
@MODES
def test_wide_groups_scratch_path(eng, monkeypatch, pos_mode, group_docs):
    """(d) the same groups over documents that hold all of a group's terms, or 65 and more of them: more than 64 pairs stay
    alive and move through the per-wave scratch region in chunks of 64 (inord_group_wide), operands of more than 64 and
    more than 128 pairs, an AND that comes out empty mid-way; operands planted in order and out of order"""
    fam = T.family_scratch()
    run(eng, monkeypatch, fam, pos_mode, group_docs)
    assert n_host_exprs(eng) == 0


@MODES
def test_long_documents(eng, monkeypatch, pos_mode):
    """(e) documents of 30 000 to 300 000 bytes, on either side of the 8-unit switch of wave_succ_min: successor in the
    threshold's unit, in the next one, five and more units on, none; a 40-byte term that starts in front of a step's last
    slice border and ends behind it; narrow chains and OR groups, wide groups compacted and through scratch"""
    fam = T.family_long()
    run(eng, monkeypatch, fam, pos_mode, None)
    assert n_host_exprs(eng) == 0


@pytest.mark.parametrize("group_docs", [None, "0"])
@MODES
def test_caller_supplied_matches_inside_groups(eng, monkeypatch, pos_mode, group_docs):
    """(f) extra literals (slots behind the dictionary's, ascending lists: they stay on the device) mixed with dictionary
    terms under OR and AND, narrow and wide, short documents and two long ones; named rows: the caller's match as the only
    successor, at the very position of a dictionary match, and a literal that is absent from the map"""
    fam = T.family_extra()
    got = run(eng, monkeypatch, fam, pos_mode, group_docs)
    assert n_host_exprs(eng) == 0
    check_named(fam, got, pos_mode)
