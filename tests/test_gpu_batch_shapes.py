"""Batches of a shape no other module reaches (batch_shapes.py; test_batch_shapes_host.py shows on the CPU that they are what
they claim to be), through the public Engine / Finder API against the oracle, whole arrays bit for bit.

A. 1 052 673 short documents: every launch_exclusive_scan of the library (document -> unit base, unit -> CSR offset, unique
   terms, the two scans of the rune pipeline, sparse row offsets, the two scans of the lowering) takes a second round of
   k_scan_spine with its carry, and every per-document kernel sees more than 2^20 documents.
B. work units with a constructed number and layout of matches at the limits of k_gather_sorted."""
import numpy as np
import pytest
import torch  # noqa: F401  (before libgft.so is loaded: both must share ONE HIP runtime, the one torch brings along)

import batch_shapes as S
from gofindthem_amd import _lib
from gofindthem_amd.engine import Engine, compact_host
from gofindthem_amd.finder import EmptyRgxEngine, Finder, GpuEngine
from helpers import assert_csr_equal
from oracle.pyoracle import POS_END, POS_START
from test_gpu_parity import KERNELS

pytestmark = pytest.mark.gpu

MODES = pytest.mark.parametrize("pos_mode", S.POS_MODES, ids=["start", "end"])
VARIANTS = pytest.mark.parametrize("variant", ["full", "holes"])
GUARD = 256
NAMED = (S.SCAN_TILE, S.BORDER, S.BORDER + 1, S.N_BIG)      # documents whose offsets an assertion message names


@pytest.fixture(scope="module")
def eng():
    e = Engine()
    yield e
    e.close()


class Big:
    """the inputs of part A, made once: index arrays, text and offsets on the host and (64 bytes of slack behind the text)
    on the device; expansions of the expectation as they are first asked for"""

    def __init__(self):
        self.x = S.Expected()
        self.idx, self.host, self.dev, self._memo = {}, {}, {}, {}
        for v in ("full", "holes"):
            self.idx[v] = S.index_array(v)
            self.host[v] = self.x.text(self.idx[v])
            self.dev[v] = self.upload(*self.host[v])

    @staticmethod
    def upload(blob, off):
        return (torch.from_numpy(np.concatenate([blob, np.zeros(64, np.uint8)])).cuda(), torch.from_numpy(off.astype(np.int64)).cuda())

    def want(self, what, variant, *args):
        key = (what, variant) + args
        if key not in self._memo:
            self._memo[key] = getattr(self.x, what)(self.idx[variant], *args)
        return self._memo[key]


@pytest.fixture(scope="module")
def big():
    return Big()


@pytest.fixture(params=["default", "dfa"])
def kernel(request, monkeypatch):
    """the default kernel's slabs go through k_gather_sorted, the DFA kernel's through k_gather; the variable is read by
    gft_build, so every test builds its dictionary after this"""
    if request.param == "default":
        monkeypatch.delenv("GFT_SCAN_KERNEL", raising=False)
    else:
        monkeypatch.setenv("GFT_SCAN_KERNEL", request.param)
    monkeypatch.delenv("GFT_SCAN_ORDERED", raising=False)
    return request.param


def build_a(eng, kernel, **kw):
    """part A's dictionary on the parametrised kernel; which gather the slabs go through hangs on the kernel the build chose"""
    eng.build(S.TERMS_A, **kw)
    assert (_lib.load().gft_scan_kernel(eng._h).decode() == "dfa") == (kernel == "dfa")


def check_csr(got, want, what):
    assert got[0].shape == want[0].shape, what
    if not np.array_equal(got[0], want[0]):
        bad = int(np.nonzero(got[0] != want[0])[0][0])
        raise AssertionError("%s: offsets differ from document %d on; at documents %s they are %s, expected %s" % (
            what, bad, list(NAMED), got[0][list(NAMED)].tolist(), want[0][list(NAMED)].tolist()))
    assert_csr_equal(got, want)


# ---- A ------------------------------------------------------------------------------------------------------------------------
@VARIANTS
@MODES
def test_scan_of_more_than_2_20_documents(eng, big, kernel, variant, pos_mode):
    build_a(eng, kernel, pos_end=(pos_mode == POS_END))
    blob, off = big.host[variant]
    check_csr(eng.scan(blob, off), big.want("scan", variant, pos_mode), "scan")


@VARIANTS
def test_unique_terms_of_more_than_2_20_documents(eng, big, kernel, variant):
    build_a(eng, kernel)
    blob, off = big.host[variant]
    got = eng.scan(blob, off, unique=True)
    check_csr(got, big.want("unique", variant), "unique")
    assert not got[2].any()


@VARIANTS
def test_rune_offsets_of_more_than_2_20_documents(eng, big, kernel, variant):
    build_a(eng, kernel)
    blob, off = big.host[variant]
    if variant == "full":
        assert int(((np.diff(off.astype(np.int64)) + S.RUNE_BLOCK - 1) // S.RUNE_BLOCK).sum()) > S.BORDER
    want = big.want("runes", variant)
    assert not np.array_equal(want[2], big.want("scan", variant, POS_START)[2])          # (the mapping does something)
    check_csr(eng.scan(blob, off, runes=True), want, "runes")


@VARIANTS
def test_to_lower_of_more_than_2_20_documents(eng, big, kernel, variant):
    """count only, then the writing call, as test_gpu_tolower.lower.  (The lowering does not read the scan kernel: the two
    parameters run the same code.)"""
    t, o = big.dev[variant]
    want, want_off = big.want("lower", variant)
    out_off = torch.full((S.N_BIG + 1,), 0x5A5A, dtype=torch.int64, device="cuda")
    total = eng.to_lower_device(t.data_ptr(), o.data_ptr(), S.N_BIG, None, 0, out_off.data_ptr())
    counted = out_off.cpu().numpy().astype(np.uint64)
    assert total == want.size
    assert np.array_equal(counted, want_off), ("count only", counted[list(NAMED)].tolist(), want_off[list(NAMED)].tolist())
    out = torch.full((total + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    out_off.fill_(0x5A5A)
    assert eng.to_lower_device(t.data_ptr(), o.data_ptr(), S.N_BIG, out.data_ptr(), total, out_off.data_ptr()) == total
    got_off = out_off.cpu().numpy().astype(np.uint64)
    assert np.array_equal(got_off, want_off), ("writing call", got_off[list(NAMED)].tolist(), want_off[list(NAMED)].tolist())
    got = out.cpu().numpy()
    if not np.array_equal(got[:total], want):
        i = int(np.nonzero(got[:total] != want)[0][0])
        raise AssertionError("byte %d (document %d) of the lower-case text differs" % (i, int(np.searchsorted(want_off, i, side="right")) - 1))
    assert (got[total:] == 0xA5).all(), "bytes stored past cap"


@VARIANTS
def test_process_and_sparse_rows_of_more_than_2_20_documents(eng, big, kernel, variant):
    build_a(eng, kernel)
    eng.set_programs(S.programs(S.EXPRS_A, eng.term_id, eng.n_terms))
    blob, off = big.host[variant]
    want = big.want("bitmap", variant)
    got = eng.process(blob, off)
    assert got.shape == want.shape
    if not np.array_equal(got, want):
        bad = np.nonzero((got != want).any(axis=1))[0]
        raise AssertionError("%d rows differ, the first at documents %s: %s, expected %s" % (bad.size, bad[:5], got[bad[:5], 0], want[bad[:5], 0]))
    ro, ei, _ = eng.process_sparse(blob, off)
    hro, hei, _, total = compact_host(want, len(S.EXPRS_A))
    assert total > S.BORDER and int(hro[S.BORDER]) > 0
    assert np.array_equal(ro, hro), ("row_off", ro[list(NAMED)].tolist(), hro[list(NAMED)].tolist())
    assert np.array_equal(ei, hei)


def test_finder_device_path_with_more_than_2_20_documents(big, kernel):
    """four synchronous batches (from the third on the unit table is k_units_single's, over N documents), a Begin / End pair,
    then the same batch with document 2^20 of 20 000 bytes: the single-unit assumption misses and the batch runs again
    through k_unit_count, the prefix sum, k_unit_fill and k_clamp_u64; then the plain batch once more.  Which batches take
    which path is the library's choice (gft_process_device: two single-unit batches in a row arm k_units_single) and is
    not observable here; every bitmap is compared whatever the path, but if that rule changes, so does what this covers."""
    from oracle.pyoracle import Oracle
    t, o = big.dev["full"]
    want = big.want("bitmap", "full")
    lblob, loff = S.with_long_document(*big.host["full"], S.BORDER)
    lt, lo = Big.upload(lblob, loff)
    orc = Oracle(S.TERMS_A, POS_START)
    orc.set_expressions(S.EXPRS_A, True)
    lwant = want.copy()
    lwant[S.BORDER] = orc.process(np.frombuffer(S.long_document(), np.uint8), np.asarray([0, S.LONG_DOC_LEN], np.uint64))[0]
    f = Finder(GpuEngine(), EmptyRgxEngine(), True)
    try:
        f.AddExpressions(S.EXPRS_A)
        bm = torch.zeros((S.N_BIG, 1), dtype=torch.int32, device="cuda")

        def check(expect, what):
            got = bm.cpu().numpy().astype(np.uint32)
            if not np.array_equal(got, expect):
                bad = np.nonzero((got != expect).any(axis=1))[0]
                raise AssertionError("%s: %d rows differ, the first at documents %s: %s, expected %s" % (what, bad.size, bad[:5], got[bad[:5], 0], expect[bad[:5], 0]))

        for k in range(4):
            bm.zero_()
            f.ProcessDevice(t.data_ptr(), o.data_ptr(), S.N_BIG, bm.data_ptr())
            check(want, "ProcessDevice %d" % k)
        bm.zero_()
        f.ProcessDeviceBegin(t.data_ptr(), o.data_ptr(), S.N_BIG, bm.data_ptr())
        f.ProcessDeviceEnd()
        check(want, "ProcessDeviceBegin / End")
        bm.zero_()
        f.ProcessDevice(lt.data_ptr(), lo.data_ptr(), S.N_BIG, bm.data_ptr())
        check(lwant, "the batch with a long document")
        bm.zero_()
        f.ProcessDevice(t.data_ptr(), o.data_ptr(), S.N_BIG, bm.data_ptr())
        check(want, "the batch after it")
        assert f.lowered_batches() == (0, 0)
    finally:
        f.close()


# ---- B ------------------------------------------------------------------------------------------------------------------------
_FAMILY, _WANT = {}, {}


def family(name, pos_mode):
    """-> (family, blob, doc_off, the oracle's CSR, its unique form): computed once, shared by the kernels"""
    if name not in _FAMILY:
        fam = S.FAMILIES[name]()
        _FAMILY[name] = (fam,) + fam.packed()
    fam, blob, off = _FAMILY[name]
    if (name, pos_mode) not in _WANT:
        csr = fam.oracle(pos_mode).scan(blob, off)
        _WANT[(name, pos_mode)] = (csr, fam.unique_of(csr))
    return (fam, blob, off) + _WANT[(name, pos_mode)]


@pytest.mark.parametrize("scan_kernel", KERNELS)
@MODES
@pytest.mark.parametrize("name", sorted(S.FAMILIES))
def test_units_at_the_limits_of_the_sorting_gather(eng, monkeypatch, name, pos_mode, scan_kernel):
    """every production kernel of the build; twice per dictionary: the second call runs with the unit size that the first call's
    match density taught the engine (scan5 only; scan3 and dfa keep theirs), documents may be cut differently and the result
    must not change; then the unique form (units of more than 256 matches, first occurrences in every round of k_unique_terms)"""
    monkeypatch.setenv("GFT_SCAN_KERNEL", scan_kernel.split("-")[0])
    if scan_kernel.endswith("-ordered"):
        monkeypatch.setenv("GFT_SCAN_ORDERED", "1")
    else:
        monkeypatch.delenv("GFT_SCAN_ORDERED", raising=False)
    fam, blob, off, want, want_unique = family(name, pos_mode)
    assert np.diff(want[0].astype(np.int64)).tolist() == fam.counts
    eng.build(fam.terms, pos_end=(pos_mode == POS_END))
    assert eng.terms() == sorted(fam.terms)
    if scan_kernel in ("scan5", "scan3"):
        assert _lib.load().gft_scan_kernel(eng._h).decode() == scan_kernel      # (its slabs are sorted by k_gather_sorted)
    if name == "interleave":                                                    # (more units than waves in the capped grid)
        assert S.INTERLEAVE_DOCS > S.GATHER_WAVES_PER_CU * torch.cuda.get_device_properties(0).multi_processor_count
    for _ in range(2):
        assert_csr_equal(eng.scan(blob, off), want)
    assert_csr_equal(eng.scan(blob, off, unique=True), want_unique)
