"""k_scan5 on presence-only batches (no INORD group, no CSR): the terms of a short-term record are written to the match pool
once per work unit.  Every bitmap of gft_process_device equals the oracle's, and the entries the scan wrote
(gft_debug_pool_entries) equal the model of tests/presence_once.py exactly -- through several short-term trips and
park_short's early drain, at the start of a document, over documents of several units (8 192 and 512 bytes), through the
second walk of a unit that outgrew the fifo, and on the benchmark's dictionary.  With one INORD group among the expressions
positions are wanted: every match is written, and gft_scan_device's CSR is the oracle's entry for entry."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before libgft.so is loaded: both must share ONE HIP runtime, the one torch brings along)

import presence_once as po
from helpers import assert_csr_equal, docs, scan_plan, tree_to_program
from oracle import dsl_ref
from oracle.pyoracle import Oracle

pytestmark = pytest.mark.gpu


def _engine(terms, exprs, case_sensitive=True):
    from gofindthem_amd import _lib
    from gofindthem_amd.engine import Engine
    e = Engine()
    e.build(terms)
    assert _lib.load().gft_scan_kernel(e._h).decode() == "scan5"

    def slot_of(lit):
        t = e.term_id(lit)
        assert t >= 0
        return t
    e.set_programs([tree_to_program(dsl_ref.parse(x, case_sensitive)[0], slot_of) for x in exprs])
    return e


class Setup:
    """an engine, the oracle's bitmaps and the model for one set of expressions over po.TERMS"""

    def __init__(self, inord):
        self.exprs = po.expressions(inord)
        self.eng = _engine(po.TERMS, self.exprs)
        self.oracle = Oracle(po.TERMS)
        self.oracle.set_expressions(self.exprs, True)
        self.model = po.Model(po.TERMS)
        self.inord = inord

    def unit_max(self):
        from gofindthem_amd import _lib
        um = C.c_uint32(0)
        assert _lib.load().gft_debug_learned_unit(self.eng._h, C.byref(um), None) == 0
        return um.value

    def largest_units(self):
        """a call without a match: the handle is back at units of 8 192 bytes, whatever the test before taught it"""
        self.check([po.fill(64)])
        assert self.unit_max() == 8192

    def check(self, texts, fold=False):
        """one gft_process_device call: the bitmap is the oracle's, the pool entries are the model's at the unit size the
        call runs with (every match when positions are wanted)"""
        unit_max = self.unit_max()
        blob, off = docs(texts)
        got, entries = process_device(self.eng, blob, off, fold)
        want = self.oracle.process(blob, off, fold=fold)
        assert np.array_equal(got, want), np.argwhere(got != want)[:4].tolist()
        once, matches = self.model.entries(blob, off, unit_max, fold)
        print("unit_max %d: entries %d, model %d, matches %d" % (unit_max, entries, once, matches))
        assert entries == (matches if self.inord else once)
        return entries, matches


def pool_entries(eng):
    from gofindthem_amd import _lib
    n = C.c_uint64(0)
    assert _lib.load().gft_debug_pool_entries(eng._h, C.byref(n)) == 0
    return int(n.value)


def device_batch(blob, off):
    t = torch.from_numpy(np.concatenate([blob, np.zeros(64, np.uint8)])).cuda()          # 64 bytes of readable slack
    o = torch.from_numpy(off.astype(np.int64)).cuda()
    return t, o


def process_device(eng, blob, off, fold=False):
    t, o = device_batch(blob, off)
    n = len(off) - 1
    bm = torch.zeros((n, (eng.n_exprs + 31) // 32), dtype=torch.int32, device="cuda")
    eng.process_device(t.data_ptr(), o.data_ptr(), n, bm.data_ptr(), fold=fold)
    torch.cuda.synchronize()
    return bm.cpu().numpy().view(np.uint32), pool_entries(eng)


@pytest.fixture(scope="module", params=[False, True], ids=["presence", "positions"])
def setup(request):
    s = Setup(request.param)
    yield s
    s.eng.close()


FIFO_CAP = scan_plan(po.TERMS)[1]["fifo_cap"]
CASES = po.single_unit_cases(FIFO_CAP)


@pytest.mark.parametrize("name", sorted(CASES))
def test_one_unit(setup, name):
    """a document of one unit, alone in its batch: repeats of one record (1, 2, 65 and enough for the early drain), the rule at
    the document's start in both orders, the second walk, the empty document, no short term at all"""
    setup.largest_units()
    entries, matches = setup.check([CASES[name]])
    if not setup.inord and name in ("ab_x65", "cab_x65", "second_walk"):
        assert entries < matches
    if name == "second_walk":
        assert entries > FIFO_CAP                        # (one unit of 8 000 bytes: its entries outgrow the fifo)


def test_all_cases_in_one_batch(setup):
    """the same documents side by side (waves take units of different documents in turn: the set is cleared per walk)"""
    setup.largest_units()
    setup.check([CASES[k] for k in sorted(CASES)] * 3)


@pytest.mark.parametrize("where", ["first", "last", "all"])
def test_units_of_a_long_document(setup, where):
    """a 20 000-byte document is three units on a handle that has learnt nothing and forty of 500 bytes behind a dense call
    (the two-call pattern of tests/test_gpu_long_terms.py); a term is written once per unit it occurs in"""
    doc = po.long_doc(where)
    setup.largest_units()
    setup.check([doc, b"", doc])
    setup.check([po.DENSE])
    assert setup.unit_max() == 512
    setup.check([doc, b"", doc])


def test_csr_with_positions_is_the_oracles():
    """gft_scan_device on the same documents: positions are wanted, the CSR equals Oracle.scan entry for entry and the pool
    holds every match"""
    from gofindthem_amd import _lib
    from gofindthem_amd.engine import Engine
    hip = C.CDLL("libamdhip64.so")
    texts = [CASES[k] for k in sorted(CASES)] + [po.long_doc("all")]
    blob, off = docs(texts)
    want = Oracle(po.TERMS).scan(blob, off)
    eng = Engine()
    try:
        eng.build(po.TERMS)
        t, o = device_batch(blob, off)
        n = len(texts)
        for _ in range(2):                               # (the second call runs at the unit size the first one taught)
            m = _lib.GftMatches()
            assert _lib.load().gft_scan_device(eng._h, t.data_ptr(), o.data_ptr(), n, 0, C.byref(m)) == 0
            nm = int(m.n_matches)
            assert nm == want[1].size == pool_entries(eng)
            mo = np.zeros(n + 1, np.uint64)
            ti, ps = np.zeros(nm, np.uint32), np.zeros(nm, np.uint32)
            for dst, src, nbytes in ((mo, m.match_off, 8 * (n + 1)), (ti, m.term_id, 4 * nm), (ps, m.pos, 4 * nm)):
                assert hip.hipMemcpy(C.c_void_p(dst.ctypes.data), C.c_void_p(src), C.c_size_t(nbytes), C.c_int(2)) == 0
            assert_csr_equal((mo, ti, ps), want)
    finally:
        eng.close()


def test_benchmark_dictionary():
    """bench.py's shape, small: 10 000 terms, 1 000 AND/OR/NOT expressions that reference all of them, 2 048 documents, folded.
    The entries per document are the model's (about 70 against the CSR's 143)"""
    from gofindthem_amd import _lib
    from gofindthem_amd.workload import Workload, make_expressions
    wl = Workload(10_000)
    terms = wl.terms()
    exprs = make_expressions(terms, 1_000, cover=True)
    n_docs = 2048
    blob, off = wl.docs_host(0, n_docs)
    blob = np.ascontiguousarray(blob[:int(off[-1])])
    oracle = Oracle(terms)
    oracle.set_expressions(exprs, False)
    want = oracle.process(blob, off, fold=True)
    model = po.Model(terms)
    eng = _engine(terms, exprs, case_sensitive=False)
    try:
        for _ in range(2):                               # (the second call runs deferred, at the learnt unit size)
            um = C.c_uint32(0)
            assert _lib.load().gft_debug_learned_unit(eng._h, C.byref(um), None) == 0
            got, entries = process_device(eng, blob, off, fold=True)
            assert np.array_equal(got, want)
            once, matches = model.entries(blob, off, um.value, fold=True)
            print("unit_max %d: %.1f entries per document, model %.1f, matches %.1f" % (um.value, entries / n_docs, once / n_docs, matches / n_docs))
            assert entries == once
    finally:
        eng.close()
