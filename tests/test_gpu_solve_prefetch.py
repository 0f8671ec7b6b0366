"""The solver's presence-matrix build at both prefetch depths (csrc/gft_solve.hip PF = 6 and 12, chosen by plan_solve from the
batch before or forced by GFT_SOLVE_PF_TERMS): 64 x 5 documents of one work unit each on an engine of one CU -- the dictionary is
large enough for one workgroup per CU, so ONE workgroup builds five groups in turn and the three-deep chain of prefetches (range
of units, unit, entries) wraps past the last group.  The units hold 0, 1, 15, 16, 17, 95, 96, 97, 191, 192 and 193 pool entries:
both sides of depth x 16 lanes of a team for both depths, so the registers alone, the registers with idle lanes, and the second,
dependent round of loads all run.  Every bitmap is the oracle's."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (before libgft.so is loaded: both must share ONE HIP runtime, the one torch brings along)

from helpers import docs, tree_to_program
from oracle import dsl_ref
from oracle.pyoracle import Oracle
from schema_scale import ONE_CU

pytestmark = pytest.mark.gpu

COUNTS = (0, 1, 15, 16, 17, 95, 96, 97, 191, 192, 193)
N_DOCS = 64 * 5
DOC_BYTES = 1024                                     # every document: 193 occurrences of five bytes fit; one work unit
PLANTED = [b"k%02dz" % i for i in range(40)]       # five bytes with the separator; the separator is in no keyword
# 10 400 keywords that no document holds: the presence matrix of 8 bytes per keyword then takes more than half of a CU's LDS
FILLER = [b"w%05dx" % i for i in range(10_400)]
TERMS = PLANTED + FILLER


def _q(t):
    return '"%s"' % t.decode()


def expressions():
    """no NOT, no INORD: the kernels that pipeline"""
    p = PLANTED
    e = [_q(t) for t in p]
    e += ["%s and %s" % (_q(p[i]), _q(p[(i + 1) % 40])) for i in range(0, 40, 5)]
    e += ["%s or %s" % (_q(p[i]), _q(p[(i + 20) % 40])) for i in range(0, 40, 5)]
    e += ["(%s and %s) or %s" % (_q(p[i]), _q(p[39 - i]), _q(FILLER[i])) for i in range(8)]
    return e


def document(d, n):
    """n occurrences of planted keywords, which ones depends on d, then separators up to DOC_BYTES"""
    body = b"".join(PLANTED[(7 * d + i) % 40] + b"." for i in range(n))
    assert len(body) <= DOC_BYTES
    return body + b"." * (DOC_BYTES - len(body))


def batch(counts):
    return [document(d, counts[d % len(counts)]) for d in range(N_DOCS)]


@functools.lru_cache(maxsize=None)
def expected(counts):
    o = Oracle(TERMS)
    o.set_expressions(expressions(), True)
    blob, off = docs(batch(counts))
    rows = o.process(blob, off, fold=False)
    rows.setflags(write=False)
    # not vacuous: the single-keyword columns of a document are exactly the keywords planted there
    hits = np.unpackbits(rows.view(np.uint8), axis=1, bitorder="little")[:, :40].sum(axis=1)
    assert hits.tolist() == [min(counts[d % len(counts)], 40) for d in range(N_DOCS)]
    return rows


def _engine():
    from gofindthem_amd import _lib
    from gofindthem_amd.engine import Engine
    e = Engine()
    assert _lib.load().gft_set_cu_margin(e._h, ONE_CU) == 0
    e.build(TERMS)
    ids = {}

    def slot_of(lit):
        if lit not in ids:
            ids[lit] = e.term_id(lit)
            assert ids[lit] >= 0
        return ids[lit]
    e.set_programs([tree_to_program(dsl_ref.parse(x, True)[0], slot_of) for x in expressions()])
    return e


def _state(eng):
    """(prefetch depth of the last solver launch, mean entries per unit the engine has learnt, pool entries of the last batch)"""
    from gofindthem_amd import _lib
    pf, ue, n = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
    assert _lib.load().gft_debug_last_solve_pf(eng._h, C.byref(pf), C.byref(ue)) == 0
    assert _lib.load().gft_debug_pool_entries(eng._h, C.byref(n)) == 0
    return pf.value, ue.value, int(n.value)


def _process(eng, counts):
    blob, off = docs(batch(counts))
    t = torch.from_numpy(np.concatenate([blob, np.zeros(64, np.uint8)])).cuda()
    o = torch.from_numpy(off.astype(np.int64)).cuda()
    bm = torch.zeros((N_DOCS, (eng.n_exprs + 31) // 32), dtype=torch.int32, device="cuda")
    eng.process_device(t.data_ptr(), o.data_ptr(), N_DOCS, bm.data_ptr(), fold=False)
    torch.cuda.synchronize()
    got = bm.cpu().numpy().view(np.uint32)
    want = expected(counts)
    bad = np.argwhere(got != want)
    assert not len(bad), "document %d (%d entries), bitmap word %d" % (bad[0][0], counts[bad[0][0] % len(counts)], bad[0][1])
    pf, learnt, entries = _state(eng)
    total = sum(counts[d % len(counts)] for d in range(N_DOCS))
    # every occurrence is one pool entry, every document one unit: the units hold exactly `counts`
    assert entries == total and learnt == -(-total // N_DOCS), (entries, total, learnt)
    return pf


def test_one_workgroup_builds_every_group():
    """on the host: the plan of this set on one CU is one workgroup, at either depth"""
    from gofindthem_amd import _lib
    for forced in (6, 12):
        out = (C.c_uint64 * 12)()
        assert _lib.load().gft_debug_plan_solve_pf(len(TERMS) + 1, len(expressions()), 400, 0, 0, 0, 160 * 1024, 1, N_DOCS, -1, 1, 0, forced,
                                                   C.addressof(out)) == 0
        group_docs, p_in_lds, per_cu, grid, has_kernel, pf = out[0], out[1], out[8], out[9], out[10], out[11]
        assert (group_docs, p_in_lds, per_cu, grid, has_kernel, pf) == (64, 1, 1, 1, 1, forced)


@pytest.mark.parametrize("depth", ["6", "12"])
def test_forced_depth(monkeypatch, depth):
    monkeypatch.setenv("GFT_SOLVE_PF_TERMS", depth)                  # (read when the handle is created, by gft_build and gft_set_programs)
    eng = _engine()
    try:
        for call in range(3):                                        # (counted, then deferred: the depth stays the forced one)
            assert _process(eng, COUNTS) == int(depth), call
    finally:
        eng.close()


def test_depth_follows_the_batch_before(monkeypatch):
    """nothing forced: a first batch runs at 12; behind a batch of few entries per unit the next runs at 6, whatever it holds
    itself; behind that one -- 83 entries per unit on average -- the next runs at 12 again.  The results do not change."""
    monkeypatch.delenv("GFT_SOLVE_PF_TERMS", raising=False)
    small = (0, 1, 15, 16, 17)
    eng = _engine()
    try:
        assert [_process(eng, c) for c in (small, COUNTS, COUNTS, small, small)] == [12, 6, 12, 12, 6]
    finally:
        eng.close()
