"""The solver's launch plan on the host (no GPU): csrc/solve_plan.cpp through gft_debug_plan_solve.

ROWS are the plans of the code this module replaced -- the planning block of solve_pipeline, launch_solve's switch and
launch_g's overrides --, recorded once from a copy of that code and kept as literals: plan_solve must give every one of them
(the kernel that launch_g picked is the row's G / P_LDS / PROG_LDS / RARE / DBG).  Then properties over a seeded sweep, and
the plans of the shapes that two tests of test_gpu_parity.py run, so that their "this path was taken" holds by construction."""
import numpy as np
import pytest

from solve_cases import LDS_MAX, N_CUS, compiled_shape, plan_solve

FIELDS = ("group_docs", "p_in_lds", "prog_in_lds", "rare", "dbg_variant", "tile_words", "wide_cap", "lds_bytes", "per_cu", "grid")

# n_slots, n_exprs, fprog_words, has_rare, wide_pairs, lds_max, n_cus, n_docs, forced_group, dbg,   then FIELDS.  In this order:
#   the benchmark's shape (10 000 terms, 1 000 expressions, 1 M documents), and with 50 % INORD expressions
#   every G at the largest n_slots that fits and at one more (the last: the presence matrix in HBM)
#   programs that just fit LDS and just do not (without / with rare words; with the presence matrix in HBM)
#   a wide set at every G and in HBM
#   every forced group: unset, 64, 32, 16, 8, "0", a width that does not exist, widths that do not fit
#   GFT_SOLVE_DEBUG: the two shapes with a DBG variant (each without / with rare words), and shapes without one
#   document counts: 1, group_docs - 1, group_docs, group_docs + 1 (G = 64 and 8), either side of the grid cap, few CUs
#   a device with 64 KiB of LDS; many expressions (several tiles), one expression, tile edges
ROWS = [
    (10001, 1000, 7372, 0, 0, 163840, 256, 1000000, -1, 0,  64, 1, 1, 0, 0, 32, 0, 134148, 1, 256),
    (10001, 1000, 7640, 1, 0, 163840, 256, 1000000, -1, 0,  64, 1, 1, 1, 0, 32, 0, 135220, 1, 256),
    (18272, 1000, 6000, 0, 0, 163840, 256, 200000, -1, 0,  64, 1, 0, 0, 0, 32, 0, 162816, 1, 256),
    (18273, 1000, 6000, 0, 0, 163840, 256, 200000, -1, 0,  32, 1, 1, 0, 0, 32, 0, 121748, 1, 256),
    (36544, 1000, 6000, 0, 0, 163840, 256, 200000, -1, 0,  32, 1, 0, 0, 0, 32, 0, 162816, 1, 256),
    (36545, 1000, 6000, 0, 0, 163840, 256, 200000, -1, 0,  16, 1, 1, 0, 0, 32, 0, 121748, 1, 256),
    (73088, 1000, 6000, 0, 0, 163840, 256, 200000, -1, 0,  16, 1, 0, 0, 0, 32, 0, 162816, 1, 256),
    (73089, 1000, 6000, 0, 0, 163840, 256, 200000, -1, 0,  8, 1, 1, 0, 0, 32, 0, 121748, 1, 256),
    (146176, 1000, 6000, 0, 0, 163840, 256, 200000, -1, 0,  8, 1, 0, 0, 0, 32, 0, 162816, 1, 256),
    (146177, 1000, 6000, 0, 0, 163840, 256, 200000, -1, 0,  64, 0, 1, 0, 0, 32, 0, 48644, 3, 768),
    (1001, 200, 37403, 0, 0, 163840, 256, 200000, -1, 0,  64, 1, 1, 0, 0, 7, 0, 162816, 1, 256),
    (1001, 200, 37404, 0, 0, 163840, 256, 200000, -1, 0,  64, 1, 0, 0, 0, 7, 0, 11600, 8, 2048),
    (1001, 200, 37403, 1, 0, 163840, 256, 200000, -1, 0,  64, 1, 1, 1, 0, 7, 0, 162816, 1, 256),
    (1001, 200, 37404, 1, 0, 163840, 256, 200000, -1, 0,  64, 1, 0, 1, 0, 7, 0, 11600, 8, 2048),
    (200000, 200, 39407, 0, 0, 163840, 256, 200000, -1, 0,  64, 0, 1, 0, 0, 7, 0, 162816, 1, 256),
    (200000, 200, 39408, 1, 0, 163840, 256, 200000, -1, 0,  64, 0, 0, 1, 0, 7, 0, 3584, 8, 2048),
    (1000, 300, 2500, 1, 100, 163840, 256, 200000, -1, 0,  64, 1, 0, 2, 0, 10, 128, 13376, 8, 2048),
    (20000, 300, 2500, 1, 100, 163840, 256, 200000, -1, 0,  32, 1, 0, 2, 0, 10, 128, 85376, 1, 256),
    (40000, 300, 2500, 1, 100, 163840, 256, 200000, -1, 0,  16, 1, 0, 2, 0, 10, 128, 85376, 1, 256),
    (100000, 300, 2500, 1, 100, 163840, 256, 200000, -1, 0,  8, 1, 0, 2, 0, 10, 128, 105376, 1, 256),
    (200000, 300, 2500, 1, 100, 163840, 256, 200000, -1, 0,  64, 0, 0, 2, 0, 10, 128, 5376, 8, 2048),
    (1000, 300, 2500, 0, 8192, 163840, 256, 200000, -1, 0,  64, 1, 0, 2, 0, 10, 8192, 13376, 8, 2048),
    (1001, 200, 1500, 1, 0, 163840, 256, 403, -1, 0,  64, 1, 1, 1, 0, 7, 0, 19204, 8, 7),
    (1001, 200, 1500, 1, 0, 163840, 256, 403, 64, 0,  64, 1, 1, 1, 0, 7, 0, 19204, 8, 7),
    (1001, 200, 1500, 1, 0, 163840, 256, 403, 32, 0,  32, 1, 1, 1, 0, 7, 0, 15204, 8, 13),
    (1001, 200, 1500, 1, 0, 163840, 256, 403, 16, 0,  16, 1, 1, 1, 0, 7, 0, 13204, 8, 26),
    (1001, 200, 1500, 1, 0, 163840, 256, 403, 8, 0,  8, 1, 1, 1, 0, 7, 0, 12196, 8, 51),
    (1001, 200, 1500, 1, 0, 163840, 256, 403, 0, 0,  64, 0, 1, 1, 0, 7, 0, 11188, 8, 7),
    (1001, 200, 1500, 1, 0, 163840, 256, 403, 5, 0,  64, 0, 1, 1, 0, 7, 0, 11188, 8, 7),
    (20000, 200, 1500, 0, 0, 163840, 256, 200000, 64, 0,  64, 0, 1, 0, 0, 7, 0, 11188, 8, 2048),
    (20000, 200, 1500, 0, 0, 163840, 256, 200000, 16, 0,  16, 1, 1, 0, 0, 7, 0, 51188, 3, 768),
    (2001, 12000, 90000, 1, 0, 163840, 256, 150, 16, 0,  16, 1, 0, 1, 0, 64, 0, 37040, 4, 10),
    (10001, 1000, 7372, 0, 0, 163840, 256, 200000, -1, 8,  64, 1, 1, 0, 1, 32, 0, 134148, 1, 256),
    (10001, 1000, 7640, 1, 0, 163840, 256, 200000, -1, 1,  64, 1, 1, 1, 1, 32, 0, 135220, 1, 256),
    (100001, 1000, 50000, 0, 0, 163840, 256, 200000, -1, 8,  8, 1, 0, 0, 1, 32, 0, 116656, 1, 256),
    (100001, 1000, 50000, 1, 0, 163840, 256, 200000, -1, 2,  8, 1, 0, 1, 1, 32, 0, 116656, 1, 256),
    (20000, 1000, 6000, 0, 0, 163840, 256, 200000, -1, 8,  32, 1, 1, 0, 0, 32, 0, 128644, 1, 256),
    (100001, 100, 600, 0, 0, 163840, 256, 200000, -1, 8,  8, 1, 1, 0, 0, 4, 0, 105524, 1, 256),
    (1000, 300, 2500, 1, 100, 163840, 256, 200000, -1, 8,  64, 1, 0, 2, 0, 10, 128, 13376, 8, 2048),
    (200000, 1000, 6000, 0, 0, 163840, 256, 200000, -1, 8,  64, 0, 1, 0, 0, 32, 0, 48644, 3, 768),
    (1001, 200, 1500, 0, 0, 163840, 256, 1, -1, 0,  64, 1, 1, 0, 0, 7, 0, 19204, 8, 1),
    (1001, 200, 1500, 0, 0, 163840, 256, 63, -1, 0,  64, 1, 1, 0, 0, 7, 0, 19204, 8, 1),
    (1001, 200, 1500, 0, 0, 163840, 256, 64, -1, 0,  64, 1, 1, 0, 0, 7, 0, 19204, 8, 1),
    (1001, 200, 1500, 0, 0, 163840, 256, 65, -1, 0,  64, 1, 1, 0, 0, 7, 0, 19204, 8, 2),
    (100001, 1000, 50000, 0, 0, 163840, 256, 7, -1, 0,  8, 1, 0, 0, 0, 32, 0, 116656, 1, 1),
    (100001, 1000, 50000, 0, 0, 163840, 256, 8, -1, 0,  8, 1, 0, 0, 0, 32, 0, 116656, 1, 1),
    (100001, 1000, 50000, 0, 0, 163840, 256, 9, -1, 0,  8, 1, 0, 0, 0, 32, 0, 116656, 1, 2),
    (1001, 200, 1500, 0, 0, 163840, 256, 131071, -1, 0,  64, 1, 1, 0, 0, 7, 0, 19204, 8, 2048),
    (1001, 200, 1500, 0, 0, 163840, 256, 131073, -1, 0,  64, 1, 1, 0, 0, 7, 0, 19204, 8, 2048),
    (1001, 200, 1500, 0, 0, 163840, 4, 5000, -1, 0,  64, 1, 1, 0, 0, 7, 0, 19204, 8, 32),
    (10001, 1000, 6000, 0, 0, 163840, 1, 1000, -1, 0,  64, 1, 1, 0, 0, 32, 0, 128660, 1, 1),
    (1001, 200, 1500, 0, 0, 65536, 256, 200000, -1, 0,  64, 1, 1, 0, 0, 7, 0, 19204, 3, 768),
    (5000, 200, 1500, 0, 0, 65536, 256, 200000, -1, 0,  64, 1, 1, 0, 0, 7, 0, 51188, 1, 256),
    (10001, 1000, 6000, 0, 0, 65536, 256, 200000, -1, 0,  32, 1, 0, 0, 0, 32, 0, 56656, 1, 256),
    (60000, 1000, 6000, 0, 0, 65536, 256, 200000, -1, 0,  64, 0, 1, 0, 0, 32, 0, 48644, 1, 256),
    (2001, 12000, 90000, 1, 0, 163840, 256, 150, -1, 0,  64, 1, 0, 1, 0, 64, 0, 49040, 3, 3),
    (9, 1, 4, 0, 0, 163840, 256, 200000, -1, 0,  64, 1, 1, 0, 0, 1, 0, 620, 8, 2048),
    (9, 33, 140, 1, 0, 163840, 256, 200000, -1, 0,  64, 1, 1, 1, 0, 2, 0, 2188, 8, 2048),
    (101, 2048, 9000, 0, 0, 163840, 256, 200000, -1, 0,  64, 1, 1, 0, 0, 64, 0, 86228, 1, 256),
    (101, 2049, 9000, 0, 0, 163840, 256, 200000, -1, 0,  64, 1, 1, 0, 0, 64, 0, 86236, 1, 256),
]


def test_the_table_covers_what_it_should():
    assert len(ROWS) >= 40
    plans = [dict(zip(FIELDS, r[10:])) for r in ROWS]
    widths = {(64, 1), (32, 1), (16, 1), (8, 1), (64, 0)}
    assert {(p["group_docs"], p["p_in_lds"]) for p in plans} == widths
    assert {(p["group_docs"], p["p_in_lds"]) for p in plans if p["rare"] == 2} == widths
    assert {r[8] for r in ROWS} >= {-1, 64, 32, 16, 8, 0}
    assert {(p["group_docs"], p["prog_in_lds"]) for p in plans if p["dbg_variant"]} == {(64, 1), (8, 0)}
    assert any(r[9] and not p["dbg_variant"] for r, p in zip(ROWS, plans))
    assert any(p["grid"] == r[6] * p["per_cu"] for r, p in zip(ROWS, plans)) and any(p["grid"] == 1 for p in plans)


@pytest.mark.parametrize("row", ROWS, ids=lambda r: "-".join(str(x) for x in r[:10]))
def test_recorded_plans(row):
    n_slots, n_exprs, fprog_words, has_rare, wide_pairs, lds_max, n_cus, n_docs, forced, dbg = row[:10]
    got = plan_solve(n_slots, n_exprs, fprog_words, has_rare, wide_pairs, lds_max, n_cus, n_docs, forced_group=forced, dbg=dbg)
    assert tuple(got[f] for f in FIELDS) == tuple(row[10:])
    assert got["has_kernel"] == 1


def test_properties_over_a_sweep():
    rng = np.random.default_rng(20)
    seen = set()
    for _ in range(4000):
        lds_max = int(rng.choice([64, 96, 160])) * 1024
        n_slots = int(rng.choice([rng.integers(2, 3000), rng.integers(2, 200000), rng.integers(2, 2000000)]))
        n_exprs = int(rng.choice([rng.integers(1, 70), rng.integers(1, 3000), rng.integers(1, 20000)]))
        fprog_words = 4 * int(n_exprs * rng.integers(1, 12))
        has_rare, wide = int(rng.integers(2)), int(rng.choice([0, 0, 0, 65, 8192]))
        n_cus, n_docs = int(rng.choice([1, 8, 256, 304])), int(rng.choice([1, 7, 63, 64, 65, 1000, 10 ** 6, 10 ** 7]))
        forced, prog_lds, dbg = int(rng.choice([-1, -1, -1, 64, 32, 16, 8, 0, 5])), int(rng.integers(4) != 0), int(rng.choice([0, 0, 8]))
        p = plan_solve(n_slots, n_exprs, fprog_words, has_rare, wide, lds_max, n_cus, n_docs, forced, prog_lds, dbg)
        case = (n_slots, n_exprs, fprog_words, has_rare, wide, lds_max, n_cus, n_docs, forced, prog_lds, dbg, p)
        assert p["lds_bytes"] <= lds_max, case
        assert not (wide and p["prog_in_lds"]), case
        assert p["rare"] == (2 if wide else has_rare) and p["wide_cap"] >= wide and p["wide_cap"] % 64 == 0, case
        assert p["p_in_lds"] or p["group_docs"] == 64, case
        assert p["group_docs"] in (64, 32, 16, 8) and (forced < 0 or not p["p_in_lds"] or p["group_docs"] == forced), case
        assert prog_lds or not p["prog_in_lds"], case
        assert dbg or not p["dbg_variant"], case
        assert 1 <= p["grid"] <= n_cus * p["per_cu"] and 1 <= p["per_cu"] <= 8, case
        assert p["grid"] == min((n_docs + p["group_docs"] - 1) // p["group_docs"], n_cus * p["per_cu"]), case
        assert p["has_kernel"] == 1, case
        seen.add((p["group_docs"], p["p_in_lds"], p["prog_in_lds"], p["rare"], p["dbg_variant"]))
    assert len(seen) == 29                       # every kernel the library carries is some plan's


def _parity_shape(n_terms, n_exprs, inord):
    """the program set that test_gpu_parity.py builds from these numbers (its _programs: term id = index in the oracle's
    term list, which `both` asserts to be the engine's)"""
    from gofindthem_amd.workload import Workload, make_expressions
    from helpers import tree_to_program
    from oracle import dsl_ref
    from oracle.pyoracle import Oracle
    terms = Workload(n_terms).terms()
    tid = {t: i for i, t in enumerate(Oracle(terms).terms())}
    exprs = make_expressions(terms, n_exprs, inord_fraction=inord)
    progs = [tree_to_program(dsl_ref.parse(e, False)[0], lambda lit: tid[lit.encode()]) for e in exprs]
    return len(tid) + 1, progs


@pytest.mark.parametrize("group_docs", [None, "16"])
def test_many_expressions_plan_programs_in_global_memory(group_docs):
    n_slots, progs = _parity_shape(2000, 12000, 0.2)         # test_many_expressions_programs_in_global_memory
    s = compiled_shape(progs, n_slots)
    p = plan_solve(n_slots, len(progs), s["fprog_words"], s["has_rare"], s["wide_pairs"], LDS_MAX, N_CUS, 150,
                   forced_group=-1 if group_docs is None else int(group_docs))
    assert p["prog_in_lds"] == 0 and p["p_in_lds"] == 1 and p["group_docs"] == (64 if group_docs is None else 16)
    assert p["tile_words"] == 64 and len(progs) > 32 * 64    # several output tiles per group


def test_group_width_zero_plans_the_presence_matrix_in_hbm():
    n_slots, progs = _parity_shape(1000, 200, 0.4)           # test_solver_group_widths
    s = compiled_shape(progs, n_slots)
    for forced, want in ((32, (32, 1)), (16, (16, 1)), (8, (8, 1)), (0, (64, 0))):
        p = plan_solve(n_slots, len(progs), s["fprog_words"], s["has_rare"], s["wide_pairs"], LDS_MAX, N_CUS, 403, forced_group=forced)
        assert (p["group_docs"], p["p_in_lds"]) == want
