"""k_scan5 at the boundary between two work units (tests/unit_boundaries.py) on ONE CU: the 16 waves of one workgroup walk all
units, each goes from the flush of one unit to the first bytes of its next, and the last ones have no next unit.
Every batch runs through gft_scan_device -- the CSR is the oracle's, position for position -- and through gft_process_device --
the presence-only bitmap of placement.py's expressions is the oracle's --, with and without folding; expectations are computed
on the bare documents and know nothing of lead bytes or slack."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before libgft.so is loaded: both must share ONE HIP runtime, the one torch brings along)

import unit_boundaries as ub
from helpers import assert_csr_equal, tree_to_program
from oracle import dsl_ref
from schema_scale import ONE_CU

pytestmark = pytest.mark.gpu

FOLD = 1                                                 # GFT_FOLD_ASCII
AT = 3                                                   # the text pointer's residue on the 16-byte grid


@pytest.fixture(scope="module")
def hip():
    return C.CDLL("libamdhip64.so")


def _engine(monkeypatch):
    from gofindthem_amd import _lib
    from gofindthem_amd.engine import Engine
    monkeypatch.delenv("GFT_SCAN_KERNEL", raising=False)
    e = Engine()
    assert _lib.load().gft_set_cu_margin(e._h, ONE_CU) == 0
    e.build(ub.TERMS)
    assert _lib.load().gft_scan_kernel(e._h).decode() == "scan5"
    ids = {t.decode(): i for i, t in enumerate(sorted(set(ub.TERMS)))}
    e.set_programs([tree_to_program(dsl_ref.parse(x, True)[0], lambda lit: ids[lit]) for x in ub.EXPRESSIONS])
    return e


class Placed:
    def __init__(self, name):
        buf, off, start = ub.placed(name, AT)
        self.t = torch.from_numpy(buf).cuda()
        self.o = torch.from_numpy(off.astype(np.int64)).cuda()
        self.n = len(off) - 1
        self.text, self.off = self.t.data_ptr() + start, self.o.data_ptr()


def _download(hip, ptr, dtype, n):
    a = np.zeros(max(n, 1), dtype=dtype)
    if n:
        assert hip.hipMemcpy(C.c_void_p(a.ctypes.data), C.c_void_p(ptr), C.c_size_t(a.itemsize * n), C.c_int(2)) == 0
    return a[:n]


def _scan(hip, eng, p, fold):
    from gofindthem_amd._lib import GftMatches
    m = GftMatches()
    eng._check(eng._L.gft_scan_device(eng._h, p.text, p.off, p.n, FOLD if fold else 0, C.byref(m)))
    nm = int(m.n_matches)
    return _download(hip, m.match_off, np.uint64, p.n + 1), _download(hip, m.term_id, np.uint32, nm), _download(hip, m.pos, np.uint32, nm)


def _process(eng, p, fold):
    bm = torch.zeros((p.n, (len(ub.EXPRESSIONS) + 31) // 32), dtype=torch.int32, device="cuda")
    eng.process_device(p.text, p.off, p.n, bm.data_ptr(), fold=fold)
    torch.cuda.synchronize()
    return bm.cpu().numpy().view(np.uint32)


def _unit_max(eng):
    um = C.c_uint32(0)
    assert eng._L.gft_debug_learned_unit(eng._h, C.byref(um), None) == 0
    return um.value


def _check_rows(got, name, fold, what):
    want = ub.expected_rows(name, fold)
    rows = np.nonzero((got != want).any(axis=1))[0]
    assert not rows.size, "%s: %d rows differ, the first %s" % (what, rows.size, rows[:6].tolist())


@pytest.mark.parametrize("fold", [False, True], ids=["raw", "fold"])
@pytest.mark.parametrize("name", sorted(n for n in ub.cases() if n != "long_doc"))
def test_scan_and_process(hip, monkeypatch, name, fold):
    """one call each on a fresh engine (units of up to 8 192 bytes); a second process call runs deferred, without the blob's end"""
    p = Placed(name)
    eng = _engine(monkeypatch)
    try:
        assert_csr_equal(_scan(hip, eng, p, fold), ub.expected_csr(name, fold))
    finally:
        eng.close()
    eng = _engine(monkeypatch)
    try:
        for call in range(2):
            _check_rows(_process(eng, p, fold), name, fold, "call %d" % call)
    finally:
        eng.close()


@pytest.mark.parametrize("fold", [False, True], ids=["raw", "fold"])
def test_long_document_at_both_unit_sizes(hip, monkeypatch, fold):
    """the 40 000-byte document is five units on a fresh engine and 79 of 507 bytes on the second call of the same engine, which
    has learnt 512-byte units from the first: the next unit of a wave lies in the same document, keywords lie across every border"""
    name = "long_doc"
    p = Placed(name)
    eng = _engine(monkeypatch)
    try:
        for want_unit in ub.UNIT_SIZES:
            assert _unit_max(eng) == want_unit
            assert_csr_equal(_scan(hip, eng, p, fold), ub.expected_csr(name, fold))
        assert _unit_max(eng) == 512
    finally:
        eng.close()
    eng = _engine(monkeypatch)
    try:
        for call, want_unit in enumerate(ub.UNIT_SIZES + (512,)):
            assert _unit_max(eng) == want_unit
            _check_rows(_process(eng, p, fold), name, fold, "call %d, units of %d" % (call, want_unit))
    finally:
        eng.close()
