"""Keywords of 301 to 7 424 bytes on the device: the families of tests/long_terms.py through every scan kernel of the library
and the INORD solver, against the oracle (which tests/test_long_terms_host.py checks against a brute-force list at these
lengths).  What each test pins is a term in max_term_len that is small against a work unit in every other test: the DFA
kernel's warm-up (7 423 bytes in front of a unit of 1 025), the position bias and the look-back of the suffix-window kernels'
verification (a match begins up to fifteen 512-byte units in front of the unit it ends in, and never in front of its
document), the solver's early stop (`back` = 7 423 against slices of 500 bytes) and the order that k_gather_sorted / k_match_off
restore from positions that interleave across many units."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before libgft.so is loaded: both must share ONE HIP runtime, the one torch brings along)

import long_terms as lt
from helpers import assert_csr_equal, docs, learned_unit, tree_to_program
from inord_trees import gen_expr
from oracle import dsl_ref
from oracle.pyoracle import Oracle, POS_END, POS_START, pack_strings

pytestmark = pytest.mark.gpu


def _kernels():
    """the scan kernels of THIS build of libgft.so (as tests/test_gpu_parity.py)"""
    from gofindthem_amd import _lib
    try:
        extra = b"extra_kernels=1" in _lib.load().gft_build_info()
    except Exception:                       # (no library: the tests themselves will say so)
        extra = False
    return ["scan5", "scan3", "dfa"] + (["scan4", "scan2", "scan2-ordered"] if extra else [])


KERNELS = _kernels()


@pytest.fixture(params=KERNELS, autouse=True)
def scan_kernel(request, monkeypatch):
    monkeypatch.setenv("GFT_SCAN_KERNEL", request.param.split("-")[0])
    if request.param.endswith("-ordered"):
        monkeypatch.setenv("GFT_SCAN_ORDERED", "1")
    else:
        monkeypatch.delenv("GFT_SCAN_ORDERED", raising=False)
    return request.param


@pytest.fixture(scope="module")
def eng():
    from gofindthem_amd.engine import Engine
    e = Engine()
    yield e
    e.close()


def running_kernel(eng):
    from gofindthem_amd import _lib
    return _lib.load().gft_scan_kernel(eng._h).decode()


def build(eng, terms, pos_mode, scan_kernel):
    eng.build(terms, pos_end=(pos_mode == POS_END))
    assert running_kernel(eng) == scan_kernel.split("-")[0]             # (a-h and a few more bytes: every kernel applies)
    assert eng.terms() == sorted(set(terms))


def units_follow_the_density(scan_kernel):
    """the kernels whose unit size `learn` adapts (scan4's is fixed, and so is the ordered path's)"""
    return scan_kernel in ("scan5", "scan2")


def engine_unit(eng):
    """(bytes per work unit the engine's next call runs with, fifo entries it sizes them by): gft_debug_learned_unit reads the
    handle's own learnt state"""
    from gofindthem_amd import _lib
    um, fifo = C.c_uint32(0), C.c_uint32(0)
    assert _lib.load().gft_debug_learned_unit(eng._h, C.byref(um), C.byref(fifo)) == 0
    return um.value, fifo.value


def assert_next_call_runs_at_512(eng, scan_kernel, total, text_bytes):
    """after a dense call on a kernel that adapts its units: the HANDLE says 512 bytes -- and that is what `learn` makes of the
    call's match count over its text with the handle's fifo size (the engine learnt from this batch and nothing else)"""
    if not units_follow_the_density(scan_kernel):
        return
    unit, fifo = engine_unit(eng)
    assert unit == 512
    assert learned_unit(scan_kernel, fifo, total, 0, text_bytes) == 512


# ---- scans -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", lt.LENGTHS)
@pytest.mark.parametrize("name", lt.FAMILIES)
def test_scan_is_the_oracles(eng, scan_kernel, name, L):
    """gft_scan's CSR (match_off, term ids, positions) of every family at every length, start and end positions.  `planted` and
    `periodic` twice on the same engine: on the kernels that adapt their units the second call runs at 512 bytes, where a
    keyword of 7 424 bytes begins fifteen units in front of the one it ends in."""
    terms, texts, fold = lt.family(name, L)
    blob, off = docs(texts)
    for pos_mode in lt.POS_MODES:
        want = lt.expected(name, L, pos_mode)
        build(eng, terms, pos_mode, scan_kernel)
        assert engine_unit(eng)[0] == 8192                                  # (a fresh dictionary starts at the largest units)
        assert_csr_equal(eng.scan(blob, off, fold=fold), want)
        if name in ("planted", "periodic"):
            assert_next_call_runs_at_512(eng, scan_kernel, int(want[1].size), int(off[-1]))
            assert_csr_equal(eng.scan(blob, off, fold=fold), want)
            assert_csr_equal(eng.scan(blob, off, fold=fold), want)


@pytest.mark.parametrize("name", ["planted", "near_misses"])
def test_scan_of_a_device_resident_batch(eng, scan_kernel, name):
    """gft_scan_device (unit table by k_unit_count / k_unit_fill, not the host's) at 7 424 bytes; the second call runs at the
    unit size the first one taught the handle (512 bytes on scan5)"""
    from gofindthem_amd import _lib
    hip = C.CDLL("libamdhip64.so")
    terms, texts, fold = lt.family(name, lt.MAX_LEN)
    blob, off = docs(texts)
    t = torch.from_numpy(np.concatenate([blob, np.zeros(64, np.uint8)])).cuda()          # 64 bytes of readable slack
    o = torch.from_numpy(off.astype(np.int64)).cuda()
    n = len(texts)
    for pos_mode in lt.POS_MODES:
        want = lt.expected(name, lt.MAX_LEN, pos_mode)
        build(eng, terms, pos_mode, scan_kernel)
        for call in range(2):
            if call:
                assert_next_call_runs_at_512(eng, scan_kernel, int(want[1].size), int(off[-1]))
            m = _lib.GftMatches()
            assert _lib.load().gft_scan_device(eng._h, t.data_ptr(), o.data_ptr(), n, 0, C.byref(m)) == 0
            nm = int(m.n_matches)
            assert nm == want[1].size
            mo = torch.empty(n + 1, dtype=torch.int64, device="cuda")
            ti = torch.empty(max(nm, 1), dtype=torch.int32, device="cuda")
            po = torch.empty(max(nm, 1), dtype=torch.int32, device="cuda")
            assert hip.hipMemcpy(C.c_void_p(mo.data_ptr()), C.c_void_p(m.match_off), C.c_size_t(8 * (n + 1)), C.c_int(3)) == 0
            assert hip.hipMemcpy(C.c_void_p(ti.data_ptr()), C.c_void_p(m.term_id), C.c_size_t(4 * nm), C.c_int(3)) == 0
            assert hip.hipMemcpy(C.c_void_p(po.data_ptr()), C.c_void_p(m.pos), C.c_size_t(4 * nm), C.c_int(3)) == 0
            got = (mo.cpu().numpy().astype(np.uint64), ti[:nm].cpu().numpy().astype(np.uint32), po[:nm].cpu().numpy().astype(np.uint32))
            assert_csr_equal(got, want)


@pytest.mark.parametrize("L", [513, lt.MAX_LEN])
def test_rune_positions_and_unique_terms(eng, scan_kernel, L):
    """GFT_POS_RUNES and GFT_SCAN_UNIQUE on `planted` with two-byte letters in the filler: positions over runes by
    oracle/runes_ref.py, and every term once per document in first-occurrence order"""
    from oracle.runes_ref import rune_index_table
    terms, texts = lt.planted(L, letters=True)
    blob, off = docs(texts)
    build(eng, terms, POS_START, scan_kernel)
    wo, wt, wp = Oracle(terms, POS_START).scan(blob, off)
    want = wp.copy()
    for d, raw in enumerate(texts):
        tab = np.asarray(rune_index_table(raw))
        lo, hi = int(wo[d]), int(wo[d + 1])
        want[lo:hi] = tab[wp[lo:hi].astype(np.int64)]
    assert (want != wp).any()
    for _ in range(2):                                                   # (second call: learnt unit size)
        mo, ti, po = eng.scan(blob, off, runes=True)
        assert np.array_equal(mo, wo) and np.array_equal(ti, wt)
        assert np.array_equal(po, want), (po[po != want][:8], want[po != want][:8])
        mo, ti, po = eng.scan(blob, off, unique=True)
        assert not po.any()
        for d in range(len(texts)):
            first = list(dict.fromkeys(wt[int(wo[d]):int(wo[d + 1])].tolist()))
            assert ti[int(mo[d]):int(mo[d + 1])].tolist() == first, d


# ---- solver ------------------------------------------------------------------------------------------------------------
def _programs(eng, exprs):
    def slot_of(lit):
        t = eng.term_id(lit)
        assert t >= 0
        return t
    return [tree_to_program(dsl_ref.parse(e, True)[0], slot_of) for e in exprs]


def _solver_exprs():
    c = lt.solver_case()
    rng = np.random.default_rng(20261018)
    pool = [lt.X, lt.S_, lt.Y, c["L"], c["M"], c["L"], b"a"]
    rand = [gen_expr(rng, pool, lambda: int(rng.integers(2, 6)), p_or=0.4, max_groups=2) for _ in range(24)]
    return c["exprs"] + rand


_SOLVER_REF = {}


def _solver_ref(pos_mode):
    """the oracle's bitmaps of the three batches, computed once per position mode"""
    if pos_mode not in _SOLVER_REF:
        c = lt.solver_case()
        short = lt.solver_short_docs()
        mixed = [x for pair in zip(c["docs"], short) for x in pair] + short[len(c["docs"]):] + [b""]
        exprs = _solver_exprs()
        o = Oracle(c["terms"], pos_mode)
        o.set_expressions(exprs, True)
        out = {}
        for key, texts in (("long", c["docs"]), ("short", short), ("mixed", mixed)):
            blob, off = docs(texts)
            out[key] = (blob, off, o.process(blob, off), int(o.scan(blob, off)[1].size))
        _SOLVER_REF[pos_mode] = out
    return _SOLVER_REF[pos_mode]


@pytest.mark.parametrize("group_docs", [None, "8", "0"])
@pytest.mark.parametrize("pos_mode", lt.POS_MODES)
def test_inord_groups_over_a_7424_byte_match(eng, scan_kernel, monkeypatch, pos_mode, group_docs):
    """k_solve_groups on tests/long_terms.py's scenario.  With start positions the first `L or s` behind `x` is the 7 424-byte
    match at 11, whose record lies in the unit where it ENDS -- thirteen 500-byte slices behind the unit that holds `s` at 600:
    the walk of a document of 8 units or more may stop only when the next slice begins more than max_term_len - 1 bytes behind
    the best candidate.  The first call on a fresh dictionary runs at the largest units (documents of fewer than 8 units on the
    suffix-window kernels: the strided walk), the later ones at what it learnt (512 bytes on scan5: the per-unit walk); then
    documents that are short at any unit size, and a batch that mixes both with empty documents."""
    if group_docs:
        monkeypatch.setenv("GFT_SOLVE_GROUP_DOCS", group_docs)
    else:
        monkeypatch.delenv("GFT_SOLVE_GROUP_DOCS", raising=False)
    c = lt.solver_case()
    ref = _solver_ref(pos_mode)
    n_g, names = c["n_groups"], c["names"]
    blob, off, want, total = ref["long"]
    # before the device is asked: the answers differ where they should (test_long_terms_host.py has the full table)
    a, a_late, a_broken = names.index("a"), names.index("a_late"), names.index("a_broken")
    if pos_mode == POS_START:
        assert want[a, 0] & 1 and not want[a_broken, 0] & 1                  # first L-or-s behind x: 11 against 600
    else:
        assert not want[a, 0] & 1 and want[a_late, 0] & 1                    # y at 300 against y at 8 000
    assert 0 < int(np.unpackbits(want.view(np.uint8)).sum()) < want.shape[0] * len(_solver_exprs())
    build(eng, c["terms"], pos_mode, scan_kernel)
    eng.set_programs(_programs(eng, _solver_exprs()))
    assert np.array_equal(eng.process(blob, off), want)
    assert_next_call_runs_at_512(eng, scan_kernel, total, int(off[-1]))
    assert lt.SOLVER_DOC // lt.unit_slice(lt.SOLVER_DOC, 512) >= 8
    for key in ("long", "short", "mixed", "long"):
        blob, off, want, _ = ref[key]
        got = eng.process(blob, off)
        assert np.array_equal(got, want), (key, np.argwhere(got != want)[:4].tolist())


# ---- finder --------------------------------------------------------------------------------------------------------------
def test_finder_with_a_7424_character_keyword(scan_kernel):
    """DSL text -> compiler -> programs -> device: Finder.ProcessTexts and ProcessDevice with a keyword of 7 424 characters in
    INORD groups, against the oracle's process"""
    from gofindthem_amd.finder import EmptyRgxEngine, Finder, GpuEngine
    c = lt.solver_case()
    exprs = c["exprs"] + ['"%s" and not "%s"' % (c["M"].decode(), c["L"].decode()), '"a" and "b" and "c"']
    texts = c["docs"] + lt.solver_short_docs()
    texts = [t.upper() if i % 3 == 0 else t for i, t in enumerate(texts)]      # the finder folds: case must not matter
    f = Finder(GpuEngine(), EmptyRgxEngine(), False)
    try:
        f.AddExpressions(exprs)
        kws = sorted(f.GetKeywords())
        assert max(len(k) for k in kws) == lt.MAX_LEN
        o = Oracle(kws)
        o.set_expressions(exprs, False)
        blob, off = pack_strings(texts)
        want = o.process(blob, off, fold=True)
        assert want.any()
        for _ in range(2):
            assert np.array_equal(f.ProcessTexts(blob=blob, doc_off=off), want)
        t = torch.from_numpy(np.concatenate([blob, np.zeros(64, np.uint8)])).cuda()
        od = torch.from_numpy(off.astype(np.int64)).cuda()
        for _ in range(3):                                   # (first call sizes the tables, the next ones run deferred)
            bm = torch.zeros(want.shape, dtype=torch.int32, device="cuda")
            f.ProcessDevice(t.data_ptr(), od.data_ptr(), len(texts), bm.data_ptr())
            assert np.array_equal(bm.cpu().numpy().astype(np.uint32), want)
    finally:
        f.close()
