"""The prefetch depth of the solver's presence-matrix build on the host (no GPU): plan_solve through
gft_debug_plan_solve_pf.  The depth is 12 slab entries per lane unless the last batch's units held at most T = 80 entries on
average (csrc/solve_plan.hpp kPfShallowEntries), the program set has no NOT / INORD word and nothing forces 12; every plan has a
kernel in the library's launch table."""
import ctypes as C

import pytest

import solve_cases as SC

T = 80                             # kPfShallowEntries
FIELDS = SC.PLAN_FIELDS + ("pf_terms",)

# (n_slots, n_exprs, fprog_words): the benchmark's set, a 100 000-term dictionary's (8 documents per group, programs in L2), a
# small one, and one whose presence matrix goes to HBM
SHAPES = {"bench": (10_001, 1_000, 12_000), "terms100k": (100_001, 1_000, 12_000), "small": (37, 200, 1_500), "hbm": (200_001, 64, 600)}


def plan(shape, has_rare=0, wide_pairs=0, unit_entries=0, forced_pf=0, forced_group=-1, prog_lds=1, dbg=0, n_docs=100_000, expect_rc=0):
    from gofindthem_amd import _lib
    n_slots, n_exprs, fprog_words = SHAPES[shape]
    out = (C.c_uint64 * len(FIELDS))()
    rc = _lib.load().gft_debug_plan_solve_pf(n_slots, n_exprs, fprog_words, has_rare, wide_pairs, unit_entries, SC.LDS_MAX, SC.N_CUS, n_docs,
                                             forced_group, prog_lds, dbg, forced_pf, C.addressof(out))
    assert rc == expect_rc, rc
    return dict(zip(FIELDS, (int(x) for x in out)))


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_depth_follows_the_last_batch(shape):
    for entries, want in ((0, 12), (1, 6), (16, 6), (71, 6), (T - 1, 6), (T, 6), (T + 1, 12), (96, 12), (97, 12), (140, 12), (1210, 12), (2**32 - 1, 12)):
        p = plan(shape, unit_entries=entries)
        assert (p["pf_terms"], p["has_kernel"], p["rare"]) == (want, 1, 0), (entries, p)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_rare_words_keep_twelve(shape):
    """the kernels with the NOT / INORD path do not pipeline: one depth, whatever the batch before held or the environment says"""
    for wide_pairs in (0, 70):
        for entries in (0, 1, T, T + 1):
            for forced in (0, 6, 12):
                p = plan(shape, has_rare=1, wide_pairs=wide_pairs, unit_entries=entries, forced_pf=forced)
                assert (p["pf_terms"], p["has_kernel"], p["rare"]) == (12, 1, 2 if wide_pairs else 1), (wide_pairs, entries, forced, p)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_forced_depth(shape):
    for entries in (0, 1, T, T + 1, 500):
        assert plan(shape, unit_entries=entries, forced_pf=6)["pf_terms"] == 6
        assert plan(shape, unit_entries=entries, forced_pf=12)["pf_terms"] == 12
    from gofindthem_amd import _lib
    plan(shape, forced_pf=8, expect_rc=_lib.GFT_E_INVALID)         # (the environment's other values mean "unset": refresh_options)


def test_every_plan_has_a_kernel():
    """both depths over every group width, programs near and far, and the timing-study variants"""
    seen = set()
    for shape in SHAPES:
        for forced_group in (-1, 64, 32, 16, 8, 0):
            for prog_lds in (1, 0):
                for dbg in (0, 8):
                    for has_rare in (0, 1):
                        for entries in (0, T, T + 1):
                            p = plan(shape, has_rare=has_rare, unit_entries=entries, forced_group=forced_group, prog_lds=prog_lds, dbg=dbg)
                            assert p["has_kernel"] == 1, p
                            assert p["pf_terms"] == (6 if entries == T and not has_rare else 12)
                            seen.add((p["p_in_lds"], p["prog_in_lds"], p["group_docs"], p["rare"], p["dbg_variant"], p["pf_terms"]))
    assert {k[5] for k in seen} == {6, 12} and {k[2] for k in seen} == {64, 32, 16, 8}
    assert any(k[4] and k[5] == 6 for k in seen) and any(not k[0] and k[5] == 6 for k in seen)


def test_the_depth_changes_nothing_else():
    """the other words of the plan are those of gft_debug_plan_solve, at either depth"""
    for shape in SHAPES:
        n_slots, n_exprs, fprog_words = SHAPES[shape]
        old = SC.plan_solve(n_slots, n_exprs, fprog_words, 0, 0, SC.LDS_MAX, SC.N_CUS, 100_000)
        for entries in (0, T, T + 1):
            p = plan(shape, unit_entries=entries)
            assert {k: p[k] for k in SC.PLAN_FIELDS} == old
