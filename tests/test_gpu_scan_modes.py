"""GFT_POS_RUNES and GFT_SCAN_UNIQUE on the device (scan_modes.py): the rune kernels at every counted-block border and document
border, the unique kernel at its rounds, waves and reused rows, both behind gft_scan and gft_scan_device, with the text at five
residues of a guarded allocation, lead bytes that end in a cut form and a slack of continuation bytes, then of lead bytes.  Every
result array is read back and compared in full, exactly, against expectations computed on the bare documents."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (before libgft.so is loaded: both must share ONE HIP runtime, the one torch brings along)

import scan_modes as sm
from helpers import assert_csr_equal
from oracle.pyoracle import POS_END, POS_START
from placement import place
from test_gpu_parity import KERNELS

pytestmark = pytest.mark.gpu

FOLD, UNIQUE, RUNES = 1, 2, 4                # GFT_FOLD_ASCII, GFT_SCAN_UNIQUE, GFT_POS_RUNES
RESIDUES = (0, 1, 3, 8, 15)
SLACKS = (0x80, 0xC3)                        # continuation bytes (they would complete a form that ends the text), then lead bytes
# lead bytes that end in a cut form: the text's first continuation bytes would complete it
LEADS = (b"", b"ab" + sm.EURO[:2], b"\xc3", b"lead bytes " + sm.CLEF[:3], b"xyz" + sm.CLEF[:1])
# every residue with both slacks; residue 0 with and without lead bytes (doc_off[0] == 0 is a placement too)
PLACEMENTS = [(at, LEADS[(i + j) % 5], slack) for i, at in enumerate(RESIDUES) for j, slack in enumerate(SLACKS)]
BARE = [(at, b"", slack) for at in RESIDUES for slack in SLACKS]              # for the cases that bring their own lead bytes


@pytest.fixture(params=KERNELS)
def scan_kernel(request, monkeypatch):
    """the scan kernels of this build (test_gpu_parity.scan_kernel); GFT_SCAN_KERNEL is read by gft_build"""
    monkeypatch.setenv("GFT_SCAN_KERNEL", request.param.split("-")[0])
    if request.param.endswith("-ordered"):
        monkeypatch.setenv("GFT_SCAN_ORDERED", "1")
    else:
        monkeypatch.delenv("GFT_SCAN_ORDERED", raising=False)
    return request.param


def _engine(terms, pos_mode=POS_START, devices=None):
    from gofindthem_amd.engine import Engine
    e = Engine(devices=devices) if devices else Engine()
    e.build(terms, pos_end=(pos_mode == POS_END))
    return e


@pytest.fixture(scope="module")
def rune_eng():
    e = _engine(sm.RUNE_TERMS)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def _hip():
    return C.CDLL("libamdhip64.so")


def _download(ptr, dtype, n):
    a = np.zeros(max(n, 1), dtype=dtype)
    if n:
        assert _hip().hipMemcpy(C.c_void_p(a.ctypes.data), C.c_void_p(ptr), C.c_size_t(a.itemsize * n), C.c_int(2)) == 0
    return a[:n]


class Placed:
    """one placement of a case's documents, uploaded once"""

    def __init__(self, case, at, lead, slack):
        lead = case.lead if case.lead is not None else lead
        tail = (case.tail or b"") + bytes([slack]) * 64
        self.buf, self.doc_off, self.at = place(case.docs, lead, tail, at)
        self.t = torch.from_numpy(self.buf).cuda()
        self.o = torch.from_numpy(self.doc_off.astype(np.int64)).cuda()
        assert self.t.data_ptr() % 16 == 0
        self.n = len(case.docs)
        self.text, self.off = self.t.data_ptr() + self.at, self.o.data_ptr()
        self.what = (case.name, at, lead.hex(), hex(slack))


def _scan_device(eng, p, flags):
    """gft_scan_device; all three result arrays read back"""
    from gofindthem_amd._lib import GftMatches
    m = GftMatches()
    eng._check(eng._L.gft_scan_device(eng._h, p.text, p.off, p.n, flags, C.byref(m)))
    nm = int(m.n_matches)
    assert int(m.n_docs) == p.n
    return _download(m.match_off, np.uint64, p.n + 1), _download(m.term_id, np.uint32, nm), _download(m.pos, np.uint32, nm)


def _scan_host(eng, p, flags):
    """gft_scan on the placed text: doc_off[0] = the lead's length, the slack behind the text is the caller's own memory"""
    return eng.scan(p.buf[p.at:], p.doc_off, fold=bool(flags & FOLD), unique=bool(flags & UNIQUE), runes=bool(flags & RUNES))


def _nonascii(eng):
    return eng._L.gft_last_nonascii(eng._h)


def _want(case, flags, pos_mode=POS_START):
    if flags & UNIQUE:
        return sm.unique_csr(case, pos_mode)
    return sm.rune_csr(case) if flags & RUNES else sm.full_csr(case, pos_mode)


def _diff(case, got, want):
    try:
        assert_csr_equal(got, want)
    except AssertionError as e:
        try:
            where = sm.differing(case, want, got)[:6]
        except Exception:                                    # (shapes differ: the message says so)
            where = []
        return "%s; documents: %s" % (e, where)
    return None


def _check(eng, case, modes, pos_mode=POS_START, placements=PLACEMENTS):
    """`case` with each flag set of `modes` through gft_scan_device at every placement, and through gft_scan at two of them"""
    fold = FOLD if case.fold else 0
    bad, n = [], 0
    for i, (at, lead, slack) in enumerate(placements):
        p = Placed(case, at, lead, slack)
        for flags in modes:
            runs = [("device", _scan_device)] + ([("host", _scan_host)] if i in (0, 3) else [])
            for name, scan in runs:
                d = _diff(case, scan(eng, p, flags | fold), _want(case, flags, pos_mode))
                n += 1
                if d:
                    bad.append((p.what, name, flags, d))
    assert not bad, "%d of %d answers differ; the first: %s" % (len(bad), n, bad[:4])
    return n


ALL_MODES = (0, RUNES, UNIQUE)


# ---- runes -----------------------------------------------------------------------------------------------------------------------
def test_block_borders_under_every_scan_kernel(scan_kernel):
    """each form at every shift across bytes 64 and 128 of its document: every production kernel's canonical CSR through both
    pipelines (and plain, so that a difference names its stage)"""
    eng = _engine(sm.RUNE_TERMS)
    try:
        _check(eng, sm.block_borders(), ALL_MODES)
    finally:
        eng.close()


def test_document_borders_lengths_and_empty_documents(rune_eng):
    """forms cut by the border between two documents, the lengths around one and two counted blocks, runs of empty documents and
    documents without a match (the binary searches over blk_base and match_off), the folded case"""
    for case in (sm.document_borders(), sm.document_lengths(), sm.empty_and_matchless(), sm.folded()):
        _check(rune_eng, case, ALL_MODES)


@pytest.mark.parametrize("n", sm.TILE_BATCHES)
def test_batches_around_the_scan_tile(rune_eng, n):
    _check(rune_eng, sm.tile_batch(n), (RUNES, UNIQUE))


def test_forms_cut_by_the_lead_bytes_and_by_the_slack(rune_eng):
    """gft_scan_device: the lead bytes end in the front of a form and the text begins with its back; the text ends in the front of
    another and the slack begins with its back.  Neither takes part in the count"""
    for case in sm.edge_cuts():
        _check(rune_eng, case, (RUNES,), placements=BARE)


def test_one_document_of_more_than_4096_counted_blocks(rune_eng):
    _check(rune_eng, sm.long_document(), (RUNES, UNIQUE))


def test_random_documents_over_the_sweep_alphabet(rune_eng):
    """2000 seeded documents of 0 to 300 bytes over the 24 bytes of the sweep, every byte a match"""
    _check(rune_eng, sm.random_documents(), (RUNES, UNIQUE))


# ---- unique ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos_mode", [POS_START, POS_END], ids=["start", "end"])
def test_unique_lists_at_the_rounds_the_waves_and_reused_rows(pos_mode):
    """match counts around 64 and the multiples of 256, first occurrences at those borders, terms that recur rounds later, lists of
    length 1 and 600, orders against the term ids; then more documents than the grid has workgroups, in batches around the scan's
    tile"""
    eng = _engine(sm.UNIQUE_TERMS, pos_mode)
    try:
        _check(eng, sm.unique_fixed(), (UNIQUE, 0), pos_mode)
        for n in sm.UNIQUE_BATCHES:
            _check(eng, sm.unique_rows(n), (UNIQUE,), pos_mode)
    finally:
        eng.close()


# ---- one engine, many calls ----------------------------------------------------------------------------------------------------------
def test_one_engine_through_a_sequence_of_modes_and_sizes():
    """plain, unique, plain, runes, unique, both, plain ... on one handle, the batches growing and shrinking: unique_pipeline swaps
    the engine's result buffers with its own, and whatever call comes next must find buffers of its size.  Runes and unique
    together: the unique lists, every position 0"""
    flags_of = {"plain": 0, "unique": UNIQUE, "runes": RUNES, "runes+unique": RUNES | UNIQUE}
    assert [n for _, n in sm.SEQUENCE[:3]] == [200, 3000, 5000] and sm.SEQUENCE[-4][1] == 200
    eng = _engine(sm.RUNE_TERMS)
    try:
        placed = {n: Placed(sm.sequence_batch(n), 3, LEADS[1], SLACKS[0]) for n in {n for _, n in sm.SEQUENCE}}
        for scan in (_scan_device, _scan_host, _scan_device):
            for step, (mode, n) in enumerate(sm.SEQUENCE):
                case, flags = sm.sequence_batch(n), flags_of[mode]
                got = scan(eng, placed[n], flags)
                d = _diff(case, got, _want(case, flags))
                assert not d, (scan.__name__, step, mode, n, d)
                if flags & UNIQUE:
                    assert not got[2].any()
    finally:
        eng.close()


def test_runes_on_an_end_position_engine_are_refused_and_the_handle_stays_good():
    from gofindthem_amd import _lib
    from gofindthem_amd.engine import GftError
    case = sm.document_lengths()
    eng = _engine(sm.RUNE_TERMS, POS_END)
    try:
        p = Placed(case, 1, LEADS[1], SLACKS[0])
        for scan in (_scan_device, _scan_host):
            assert not _diff(case, scan(eng, p, 0), sm.full_csr(case, POS_END))
            with pytest.raises(GftError) as err:
                scan(eng, p, RUNES)
            assert err.value.code == _lib.GFT_E_UNSUPPORTED
            assert not _diff(case, scan(eng, p, 0), sm.full_csr(case, POS_END)), scan.__name__
            assert not _diff(case, scan(eng, p, UNIQUE), sm.unique_csr(case, POS_END)), scan.__name__
    finally:
        eng.close()


def test_a_handle_over_two_devices_answers_as_one_device():
    """the batch's byte cut lands at a run of empty documents, beside a rune that the run's borders cut"""
    from test_gpu_multi import _devices
    one, two = _engine(sm.RUNE_TERMS), _engine(sm.RUNE_TERMS, devices=_devices())
    try:
        for case in (sm.two_device_batch(), sm.document_borders(), sm.tile_batch(sm.SCAN_TILE + 1)):
            p = Placed(case, 3, b"", SLACKS[0])
            cut = np.zeros(3, np.uint64)
            assert two._L.gft_split_docs(two._h, p.doc_off.ctypes.data, p.n, cut.ctypes.data) == 0
            if case is sm.two_device_batch():
                # (split_by_bytes cuts in front of the first document that reaches half the bytes: the second shard begins with the
                # run of empty documents, the first ends in the front half of the cut rune)
                assert int(cut[1]) == 3 and case.docs[3:9] == [b""] * 6 and case.docs[2].endswith(sm.CLEF[:2]), cut
            for flags in ALL_MODES + (RUNES | UNIQUE,):
                want = _want(case, flags)
                for name, eng in (("one device", one), ("two devices", two)):
                    d = _diff(case, _scan_host(eng, p, flags), want)
                    assert not d, (case.name, flags, name, d)
    finally:
        one.close()
        two.close()


def test_nonascii_verdict_does_not_depend_on_the_answer_mode(rune_eng):
    """gft_last_nonascii after a runes or unique call = after the plain call on the same batch and flags"""
    ascii_only = sm.make_case("ascii", [b"ABC abc", b"", b"<ab>"])
    safe = sm.make_case("fold-safe", [b"ab" + sm.E_ACUTE, b"x"])
    seen = set()
    for case in (ascii_only, safe, sm.document_lengths(), sm.folded()):
        p = Placed(case, 8, LEADS[2], SLACKS[1])
        for fold in (0, FOLD):
            for scan in (_scan_device, _scan_host):
                scan(rune_eng, p, fold)
                plain = _nonascii(rune_eng)
                seen.add((fold, plain != 0))
                for flags in (RUNES, UNIQUE, RUNES | UNIQUE):
                    scan(rune_eng, p, fold | flags)
                    assert _nonascii(rune_eng) == plain, (case.name, fold, flags, scan.__name__)
    assert (FOLD, True) in seen and (FOLD, False) in seen            # (both verdicts occurred)
