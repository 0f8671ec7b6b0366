"""The top of k_scan5's unit loop (tests/unit_chain.py) on ONE CU: the 16 waves of one workgroup take all units; each requests
its unit's first bytes, takes its next item and loads that unit's record at a clamped index, whether or not there is such a unit.
Every batch runs twice through gft_scan_device on one engine -- positions wanted, the CSR is the oracle's, entry for entry -- and
twice through gft_process_device on another -- presence only, the bitmap is the oracle's --; the second call of each runs at the
unit size the first one learnt.  With and without folding, under a dictionary of 30 byte classes and under one of 51.  The last
test outgrows the match pool, so that the batch is scanned again from what the first scan's units counted."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before libgft.so is loaded: both must share ONE HIP runtime, the one torch brings along)

import unit_chain as uc
from helpers import assert_csr_equal, tree_to_program
from oracle import dsl_ref
from oracle.pyoracle import pack_strings
from schema_scale import ONE_CU

pytestmark = pytest.mark.gpu

FOLD = 1                                                 # GFT_FOLD_ASCII


@pytest.fixture(scope="module")
def hip():
    return C.CDLL("libamdhip64.so")


def _engine(monkeypatch, which, one_cu=True):
    from gofindthem_amd import _lib
    from gofindthem_amd.engine import Engine
    monkeypatch.delenv("GFT_SCAN_KERNEL", raising=False)
    terms = uc.DICTIONARIES[which]
    assert uc.classes(terms) <= 32 if which == "small" else uc.classes(terms) > 32
    e = Engine()
    if one_cu:
        assert _lib.load().gft_set_cu_margin(e._h, ONE_CU) == 0
    e.build(terms)
    assert _lib.load().gft_scan_kernel(e._h).decode() == "scan5"
    ids = {t.decode("utf-8"): i for i, t in enumerate(sorted(set(terms)))}
    e.set_programs([tree_to_program(dsl_ref.parse(x, True)[0], lambda lit: ids[lit]) for x in uc.expressions()])
    return e


class Placed:
    def __init__(self, buf, off):
        self.t = torch.from_numpy(buf).cuda()
        self.o = torch.from_numpy(off.astype(np.int64)).cuda()
        self.n = len(off) - 1
        self.text, self.off = self.t.data_ptr(), self.o.data_ptr()
        assert self.text % 16 == 0                       # (doc_off[0] is the first document's place in the buffer AND on the 16-byte grid)


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
    bm = torch.zeros((p.n, (len(uc.expressions()) + 31) // 32), dtype=torch.int32, device="cuda")
    eng.process_device(p.text, p.off, p.n, bm.data_ptr(), fold=fold)
    torch.cuda.synchronize()
    return bm.cpu().numpy().view(np.uint32)


def _unit_max(eng):
    um = C.c_uint32(0)
    assert eng._L.gft_debug_learned_unit(eng._h, C.byref(um), None) == 0
    return um.value


def _check_rows(got, want, what):
    rows = np.nonzero((got != want).any(axis=1))[0]
    assert not rows.size, "%s: %d rows differ, the first %s" % (what, rows.size, rows[:6].tolist())


@pytest.mark.parametrize("fold", [False, True], ids=["raw", "fold"])
@pytest.mark.parametrize("which", sorted(uc.DICTIONARIES))
@pytest.mark.parametrize("name", sorted(uc.cases()))
def test_scan_and_process_twice(hip, monkeypatch, name, which, fold):
    p = Placed(*uc.placed(name)[:2])
    eng = _engine(monkeypatch, which)
    try:
        assert _unit_max(eng) == 8192
        for call in range(2):
            assert_csr_equal(_scan(hip, eng, p, fold), uc.expected_csr(name, which, fold))
    finally:
        eng.close()
    eng = _engine(monkeypatch, which)
    try:
        for call in range(2):
            _check_rows(_process(eng, p, fold), uc.expected_rows(name, which, fold), "call %d" % call)
    finally:
        eng.close()


def _scans(eng):
    ms, n = C.c_double(), C.c_uint64()
    assert eng._L.gft_profile_read(eng._h, b"scan", C.byref(ms), C.byref(n)) == 0
    return n.value


@pytest.mark.parametrize("fold", [False, True], ids=["raw", "fold"])
def test_pool_overflow_is_scanned_again(monkeypatch, fold):
    """two small batches leave the pool at its minimum; the dense one has more documents than their unit table, so its units are
    counted before the launch, and writes more entries than the pool holds: the units past the pool count 0, the cursor tells
    the host, the pool grows and the batch is scanned again.  Then the same batch once more, into the pool as it is now"""
    docs, want, entries = uc.pool_case(fold)
    assert entries > uc.POOL_MIN
    blob, off = pack_strings(docs)
    buf = np.concatenate([np.frombuffer(bytes(blob), np.uint8), np.zeros(64, np.uint8)])
    big = Placed(buf, np.asarray(off, dtype=np.uint64))
    warm = Placed(*uc.placed("n17")[:2])
    eng = _engine(monkeypatch, "small", one_cu=False)
    try:
        for call in range(2):
            _check_rows(_process(eng, warm, fold), uc.expected_rows("n17", "small", fold), "warm %d" % call)
        eng._L.gft_profile_enable(eng._h, 1)
        eng._L.gft_profile_reset(eng._h)
        _check_rows(_process(eng, big, fold), want, "the batch that outgrows the pool")
        first = _scans(eng)
        eng._L.gft_profile_enable(eng._h, 0)
        assert first >= 2, "the batch overflowed the pool and was accepted without a second scan"
        _check_rows(_process(eng, big, fold), want, "the same batch again")
    finally:
        eng.close()
