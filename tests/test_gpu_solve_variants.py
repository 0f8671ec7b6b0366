"""The solver's kernel variants (csrc/gft_solve.hip: the near and the far fetch schedule around the one interpreter body, the
three interpreter classes, RARE 0 / 1 / 2, presence matrix in LDS at 64 and 8 documents per group and in HBM) on small
inputs, gft_process against the oracle's bitmap.  Every case runs with GFT_SOLVE_PROG_LDS unset (programs staged in LDS:
run_program) and =0 (read from L2: run_program_far) over 1, 63, 64, 65 and 130 documents; which kernel a case runs is
planned on the CPU before any launch (solve_cases.plan_solve: the function the library itself calls).  The families are
solve_cases.family(rare): programs of 1, 2, 3, 4, 5, 8 and 9 chunks in one block of 64 -- every `chunks mod 4`, lanes that
finish at different trips --, and trees nested up to 7 deep, which spill past the deep interpreter's four registers."""
import numpy as np
import pytest
import torch  # noqa: F401  (before libgft.so is loaded: both must share ONE HIP runtime, the one torch brings along)

import solve_cases as SC
from oracle.pyoracle import POS_START

pytestmark = pytest.mark.gpu

COUNTS = [1, 63, 64, 65, 130]


@pytest.fixture(scope="module")
def eng():
    from gofindthem_amd.engine import Engine
    e = Engine()
    yield e
    e.close()


@pytest.mark.parametrize("group_docs", [None, "8", "0"])
@pytest.mark.parametrize("rare", [0, 1, 2])
def test_near_and_far_interpreter(eng, monkeypatch, rare, group_docs):
    fam = SC.family(rare)
    progs, n_slots = fam.programs(), len(fam.terms) + 1
    want = fam.reference(POS_START)
    # ---- on the CPU, before any launch: the cases are what they claim to be
    truth = fam.truth(POS_START)
    for n in COUNTS:
        assert 0.1 <= truth[:n].mean() <= 0.9, n                         # at least 10 % of the bits true, 10 % false
    shape = SC.compiled_shape(progs, n_slots)
    assert set(shape["blk_class"]) == {0, 1, 2}                          # blocks of all three interpreter classes
    assert (shape["has_rare"], shape["wide_pairs"] > 0) == (rare >= 1, rare == 2)
    per = [SC.one_program(fam, i) for i in range(len(progs))]
    assert {c for c, k in per if k == 0} >= SC.CHUNKS and max(c for c, k in per if k == 2) >= 64
    assert sum(k == 0 for _, k in per) >= 64 and len(progs) <= 300
    # the deep class spills: the family without rare words (every family holds its expressions) nests 7 deep, past the
    # four registers (kSolveRegStackDeep) and into deep[]
    assert set(SC.family(0).exprs) <= set(fam.exprs) and SC.stack_depths(SC.family(0)).max() >= 7 > 4
    if rare == 0:                                                        # exactly one block per class: the lengths mix inside it
        assert shape["blk_class"] == [2, 1, 0] and [k for _, k in per].count(0) == 64
    forced = -1 if group_docs is None else int(group_docs)
    for prog_lds in (1, 0):
        for n in COUNTS:
            p = SC.plan_solve(n_slots, len(progs), shape["fprog_words"], shape["has_rare"], shape["wide_pairs"], SC.LDS_MAX, SC.N_CUS, n,
                              forced_group=forced, prog_lds=prog_lds)
            assert (p["group_docs"], p["p_in_lds"]) == {None: (64, 1), "8": (8, 1), "0": (64, 0)}[group_docs]
            assert p["prog_in_lds"] == (1 if prog_lds and rare < 2 else 0) and p["rare"] == rare and p["has_kernel"] == 1
    # ---- on the device
    monkeypatch.delenv("GFT_SCAN_KERNEL", raising=False)
    if group_docs is None:
        monkeypatch.delenv("GFT_SOLVE_GROUP_DOCS", raising=False)
    else:
        monkeypatch.setenv("GFT_SOLVE_GROUP_DOCS", group_docs)
    eng.build(fam.terms)
    assert eng.terms() == fam.terms
    got = {}
    for prog_lds in (None, "0"):
        if prog_lds is None:
            monkeypatch.delenv("GFT_SOLVE_PROG_LDS", raising=False)
        else:
            monkeypatch.setenv("GFT_SOLVE_PROG_LDS", prog_lds)           # (read by gft_set_programs)
        eng.set_programs(progs)
        for n in COUNTS:
            blob, off = fam.packed(n)
            got[prog_lds, n] = eng.process(blob, off)
            bad = np.argwhere(got[prog_lds, n] != want[:n])
            assert not len(bad), "GFT_SOLVE_PROG_LDS=%s, %d documents: document %d, bitmap word %d" % (prog_lds, n, bad[0][0], bad[0][1])
    for n in COUNTS:
        assert np.array_equal(got[None, n], got["0", n])
