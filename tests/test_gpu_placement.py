"""The scan kernels and the paths behind them wherever the text lies (placement.py): at every residue of the 16-byte grid, behind
lead bytes on both sides of the kernels' thresholds (doc_off[0] != 0), with lead bytes and slack that hold the missing half of a
cut keyword, halves of runes, or the batch's own text -- on every route a batch can get its unit table by (observed through
gft_debug_last_unit_route), with two batches in flight, from host memory behind a longer batch, over two devices, and straight on
the bucket runs of a routed blob.  Every comparison is exact, against expectations computed on the bare documents."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (before libgft.so is loaded: both must share ONE HIP runtime, the one torch brings along)

import placement as pl
from helpers import assert_csr_equal, tree_to_program
from oracle import dsl_ref, runes_ref
from oracle.pyoracle import POS_END, POS_START
from test_gpu_parity import KERNELS

pytestmark = pytest.mark.gpu

FOLD, RUNES = 1, 4                           # GFT_FOLD_ASCII, GFT_POS_RUNES


@pytest.fixture(params=KERNELS, autouse=True)
def scan_kernel(request, monkeypatch):
    """every test under every scan kernel of this build (test_gpu_parity.scan_kernel); GFT_SCAN_KERNEL is read by gft_build"""
    monkeypatch.setenv("GFT_SCAN_KERNEL", request.param.split("-")[0])
    if request.param.endswith("-ordered"):
        monkeypatch.setenv("GFT_SCAN_ORDERED", "1")
    else:
        monkeypatch.delenv("GFT_SCAN_ORDERED", raising=False)
    return request.param


def _lib():
    from gofindthem_amd import _lib as lib
    return lib.load()


@functools.lru_cache(maxsize=None)
def _hip():
    return C.CDLL("libamdhip64.so")


class Placed:
    """one placement of a batch, uploaded once: the text pointer has the residue `at` on the 16-byte grid"""

    def __init__(self, name, kind, at, lead_len, docs=None, lead=None, tail=None):
        if docs is None:
            buf, off, start = pl.placed(name, kind, at, lead_len)
        else:
            buf, off, start = pl.place(docs, lead, tail, at)
        self.what = (name, kind, at, lead_len)
        self.t = torch.from_numpy(buf).cuda()
        self.o = torch.from_numpy(off.astype(np.int64)).cuda()
        assert self.t.data_ptr() % 16 == 0 and self.o.data_ptr() % 8 == 0
        self.n = len(off) - 1
        self.text, self.off = self.t.data_ptr() + start, self.o.data_ptr()


def _engine(terms, pos_mode=POS_START, which=None):
    from gofindthem_amd.engine import Engine
    e = Engine()
    e.build(terms, pos_end=(pos_mode == POS_END))
    if which is not None:
        e.set_programs(_programs(which))
    return e


@functools.lru_cache(maxsize=None)
def _trees(which):
    return [dsl_ref.parse(x, True)[0] for x in pl.expressions(which)]


def _programs(which):
    ids = {t.decode(): i for i, t in enumerate(sorted(set(pl.TERMS_ASCII)))}
    return [tree_to_program(t, lambda lit: ids[lit]) for t in _trees(which)]


def _words(which):
    return (len(pl.expressions(which)) + 31) // 32


def _download(ptr, dtype, n):
    a = np.zeros(max(n, 1), dtype=dtype)
    if n:
        assert _hip().hipMemcpy(C.c_void_p(a.ctypes.data), C.c_void_p(ptr), C.c_size_t(a.itemsize * n), C.c_int(2)) == 0
    return a[:n]


def _scan_device(eng, p, flags=0):
    from gofindthem_amd._lib import GftMatches
    m = GftMatches()
    eng._check(eng._L.gft_scan_device(eng._h, p.text, p.off, p.n, flags, C.byref(m)))
    nm = int(m.n_matches)
    return _download(m.match_off, np.uint64, p.n + 1), _download(m.term_id, np.uint32, nm), _download(m.pos, np.uint32, nm)


def _route(eng):
    name = C.c_char_p()
    assert eng._L.gft_debug_last_unit_route(eng._h, C.byref(name)) == 0
    return name.value.decode()


def _nonascii(eng):
    return eng._L.gft_last_nonascii(eng._h)


def _csr_diff(got, want):
    try:
        assert_csr_equal(got, want)
    except AssertionError as e:
        return str(e)
    return None


def _rows(bm, n):
    return bm.cpu().numpy().astype(np.uint32)[:n]


# ---- gft_scan_device ---------------------------------------------------------------------------------------------------------
def test_csr_wherever_the_text_lies():
    """gft_scan_device on DOCS_LONG at every placement, in every surrounding, with and without folding, in both position modes:
    the CSR of the bare documents.  The mixed list (non-ASCII keywords: the large alphabet, runes cut by borders) without
    folding, and its fold-safe documents with folding."""
    runs = [("long", pl.TERMS_ASCII, (False, True)), ("long_mixed", pl.TERMS_MIXED, (False,)), ("long_mixed_safe", pl.TERMS_MIXED, (True,))]
    engines = {(id(terms), m): _engine(terms, m) for terms in (pl.TERMS_ASCII, pl.TERMS_MIXED) for m in pl.POS_MODES}
    bad, n = [], 0
    try:
        for at, lead_len in pl.PLACEMENTS:
            for kind in pl.KINDS:
                for name, terms, folds in runs:
                    p = Placed(name, kind, at, lead_len)
                    for m in pl.POS_MODES:
                        for fold in folds:
                            diff = _csr_diff(_scan_device(engines[(id(terms), m)], p, FOLD if fold else 0), pl.expected_csr(name, m, fold))
                            n += 1
                            if diff:
                                bad.append((name, kind, at, lead_len, "end" if m == POS_END else "start", "fold" if fold else "raw", diff))
    finally:
        for e in engines.values():
            e.close()
    assert not bad, "%d of %d scans differ from the bare documents' CSR; the first: %s" % (len(bad), n, bad[:8])


# ---- gft_process_device on every route ----------------------------------------------------------------------------------------
ROUTE_PLACEMENTS = ((15, 23), (1, 6), (0, 7))


@pytest.mark.parametrize("which", [pl.PRESENCE, pl.POSITIONS])
@pytest.mark.parametrize("name", ["short", "long"])
def test_process_on_every_unit_route(name, which):
    """seven calls of gft_process_device in a row on one placed batch, on a fresh engine: the first is counted, the next deferred,
    and a batch of one unit per document (DOCS_SHORT) then gets its table in one launch (single) -- the routes on which the
    kernels are told nothing of the blob's end (text_hi = ~0).  Every bitmap is the oracle's for the bare documents, and once the
    sizes are learnt no batch is scanned twice."""
    want = pl.expected_rows(name, which, True)
    words, bad, seen = _words(which), [], {}
    for at, lead_len in ROUTE_PLACEMENTS:
        for kind in pl.KINDS:
            p = Placed(name, kind, at, lead_len)
            eng = _engine(pl.TERMS_ASCII, POS_START, which)
            try:
                bm = torch.zeros((p.n, words), dtype=torch.int32, device="cuda")
                routes = []
                for call in range(7):
                    if call == 3:                                    # (sizes learnt: counted, deferred -- perhaps run again --, deferred)
                        eng.profile(True)
                        eng.profile_reset()
                    bm.zero_()
                    eng.process_device(p.text, p.off, p.n, bm.data_ptr(), fold=True)
                    routes.append(_route(eng))
                    got = _rows(bm, p.n)
                    if not np.array_equal(got, want):
                        rows = np.nonzero((got != want).any(axis=1))[0]
                        bad.append((kind, at, lead_len, call, routes[-1], "%d rows differ, the first %s" % (rows.size, rows[:5].tolist())))
                scans = eng.profile_read("scan")[1]
                eng.profile(False)
            finally:
                eng.close()
            seen[(kind, at, lead_len)] = routes
            assert routes[0] == "counted" and "deferred" in routes, (kind, at, lead_len, routes)
            if name == "short":
                assert routes[-1] == "single", (kind, at, lead_len, routes)
            else:
                assert "single" not in routes and routes[-1] == "deferred", (kind, at, lead_len, routes)
            assert scans == 4, (kind, at, lead_len, routes, "calls 4 to 7 were scanned %d times" % scans)
    print("routes of %s / %s: %s" % (name, which, sorted(set(map(tuple, seen.values())))))
    assert not bad, "%d bitmaps differ from the bare documents' rows; the first: %s" % (len(bad), bad[:8])


def test_two_batches_in_flight_at_different_placements():
    """begin(A), begin(B), end, end for eight rounds: two copies of DOCS_SHORT at different residues, behind different leads"""
    L = _lib()
    want = pl.expected_rows("short", pl.POSITIONS, True)
    words = _words(pl.POSITIONS)
    a, b = Placed("short", "completes", 1, 6), Placed("short", "neighbour", 15, 23)
    eng = _engine(pl.TERMS_ASCII, POS_START, pl.POSITIONS)
    try:
        bms = [torch.zeros((p.n, words), dtype=torch.int32, device="cuda") for p in (a, b)]
        routes = []
        for rnd in range(8):
            for p, bm in zip((a, b), bms):
                bm.zero_()
            for p, bm in zip((a, b), bms):
                eng._check(L.gft_process_device_begin(eng._h, p.text, p.off, p.n, FOLD, None, bm.data_ptr()))
                routes.append(_route(eng))
            for p, bm in zip((a, b), bms):
                eng._check(L.gft_process_device_end(eng._h))
            for p, bm in zip((a, b), bms):
                assert np.array_equal(_rows(bm, p.n), want), (rnd, p.what, routes)
        assert routes[0] == "counted" and routes[-1] == "single" and routes[-2] == "single", routes
    finally:
        eng.close()


# ---- high bytes that are no text --------------------------------------------------------------------------------------------------
def test_high_bytes_outside_the_documents_cost_no_verdict():
    """Lead bytes and slack of C3 / 89 / FF around ASCII documents, folded: the answers of the bare documents, gft_last_nonascii
    0 after every call (the DFA kernel's judge is k_fold_safe, scan3 and scan5 judge in the kernel), and a Finder does not lower
    the batch.  Around documents with runes: verdict 0 while every document is safe by itself, and non-zero for a document that
    ends in a lead byte which the slack would complete or begins with a continuation byte which the lead bytes would introduce --
    strings.ToLower sees documents one by one."""
    from gofindthem_amd.finder import EmptyRgxEngine, Finder, GpuEngine
    kinds = ("rune", "ones")
    ascii_eng, mixed_eng = _engine(pl.TERMS_ASCII), _engine(pl.TERMS_MIXED)
    proc = _engine(pl.TERMS_ASCII, POS_START, pl.POSITIONS)
    f = Finder(GpuEngine(), EmptyRgxEngine(), False)
    try:
        f.AddExpressions(list(pl.expressions(pl.POSITIONS)))
        words = _words(pl.POSITIONS)
        safe = pl.batch("short_mixed_safe").docs
        ends_in_lead = safe + [b"abc 30\xc2"]                        # (C2 89 would be a sign without case)
        starts_with_continuation = [b"\xa9 au lait"] + safe          # (C3 A9 would be a lower-case letter)
        assert all(map(pl.fold_safe, safe)) and pl.fold_safe(b"\xc2\x89") and pl.fold_safe(b"\xc3\xa9")
        for at, lead_len in pl.PLACEMENTS:
            for kind in kinds:
                what = (kind, at, lead_len)
                p = Placed("long", kind, at, lead_len)
                diff = _csr_diff(_scan_device(ascii_eng, p, FOLD), pl.expected_csr("long", POS_START, True))
                assert not diff, (what, diff)
                assert _nonascii(ascii_eng) == 0, what
                p = Placed("long_mixed_safe", kind, at, lead_len)
                diff = _csr_diff(_scan_device(mixed_eng, p, FOLD), pl.expected_csr("long_mixed_safe", POS_START, True))
                assert not diff, (what, diff)
                assert _nonascii(mixed_eng) == 0, what
                if lead_len == 0 or kind != "rune":
                    continue
                lead, tail = pl.surroundings("rune", lead_len, pl.batch("short_mixed_safe"))
                for docs, why in ((ends_in_lead, "a lead byte ends the last document"), (starts_with_continuation, "a continuation byte begins the first")):
                    p = Placed(why, "rune", at, lead_len, docs=docs, lead=lead, tail=tail)
                    _scan_device(mixed_eng, p, FOLD)
                    assert _nonascii(mixed_eng) != 0, (what, why)
        # the routes of gft_process_device (deferred and single: the kernels are told nothing of the blob's end), and a Finder
        want = pl.expected_rows("short", pl.POSITIONS, True)
        for at, lead_len in ROUTE_PLACEMENTS:
            for kind in kinds:
                p = Placed("short", kind, at, lead_len)
                bm = torch.zeros((p.n, words), dtype=torch.int32, device="cuda")
                for call in range(4):
                    bm.zero_()
                    proc.process_device(p.text, p.off, p.n, bm.data_ptr(), fold=True)
                    assert np.array_equal(_rows(bm, p.n), want), (kind, at, lead_len, call, _route(proc))
                    assert _nonascii(proc) == 0, (kind, at, lead_len, call, _route(proc))
                for call in range(4):
                    bm.zero_()
                    f.ProcessDevice(p.text, p.off, p.n, bm.data_ptr())
                    assert np.array_equal(_rows(bm, p.n), want), (kind, at, lead_len, call, "finder")
                    assert f.lowered_batches() == (0, 0), (kind, at, lead_len, call)
        assert _route(proc) == "single"
    finally:
        f.close()
        for e in (ascii_eng, mixed_eng, proc):
            e.close()


# ---- from host memory ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rune_csr(name):
    """expected_csr(name, POS_START, False) with every position counted in runes of its document (oracle/runes_ref.py)"""
    mo, ti, po = pl.expected_csr(name, POS_START, False)
    out = po.copy()
    for d, doc in enumerate(pl.batch(name).docs):
        a, b = int(mo[d]), int(mo[d + 1])
        if b > a:
            t = np.asarray(runes_ref.rune_index_table(doc), dtype=np.uint32)
            out[a:b] = t[po[a:b]]
    return mo, ti, out


def test_host_path_behind_a_longer_batch():
    """gft_scan / gft_process from host memory: the staging buffer is never cleared, so behind a batch lies what a longer batch
    before it left there -- here the bytes that complete the keyword the batch's last document starts.  With lead bytes
    (doc_off[0] = 5, 16) the whole of [0, doc_off[n]) is uploaded and the rune pass's 16-byte grid moves against the documents."""
    b, mixed = pl.batch("long"), pl.batch("long_mixed")
    more = b.rest + pl.batch("short").docs[7][:200]
    for pos_mode in pl.POS_MODES:
        eng = _engine(pl.TERMS_ASCII, pos_mode, pl.POSITIONS)
        try:
            for lead_len in (0, 5):
                lead, tail = pl.surroundings("completes", lead_len, b)
                buf, off, at = pl.place(b.docs + [more], lead, tail, 3)
                eng.scan(buf[at:], off, fold=True)
                buf, off, at = pl.place(b.docs, lead, tail, 3)
                for fold in (True, False):
                    assert_csr_equal(eng.scan(buf[at:], off, fold=fold), pl.expected_csr("long", pos_mode, fold))
                    assert _route(eng) == "host"
                buf2, off2, _ = pl.place(b.docs + [more], lead, tail, 3)
                eng.process(buf2[at:], off2, fold=True)
                assert np.array_equal(eng.process(buf[at:], off, fold=True), pl.expected_rows("long", pl.POSITIONS, True)), (pos_mode, lead_len)
                assert _route(eng) == "host"
        finally:
            eng.close()
    eng = _engine(pl.TERMS_MIXED)
    try:
        want = _rune_csr("long_mixed")
        for lead_len in (0, 5, 16):
            lead, tail = pl.surroundings("rune", lead_len, mixed)
            buf, off, at = pl.place(mixed.docs + ["é".encode() * 100], lead, tail, 3)
            eng.scan(buf[at:], off, runes=True)
            buf, off, at = pl.place(mixed.docs, lead, tail, 3)
            assert_csr_equal(eng.scan(buf[at:], off, runes=True), want)
            assert _route(eng) == "host"
        for at, lead_len in ((1, 6), (15, 23)):                      # GFT_POS_RUNES on gft_scan_device (include/gft.h allows it)
            assert_csr_equal(_scan_device(eng, Placed("long_mixed", "rune", at, lead_len), RUNES), want)
    finally:
        eng.close()


def test_engine_over_two_devices_with_lead_bytes():
    """a handle over two devices cuts the batch by bytes counted from doc_off[0] and hands every shard its own offsets"""
    from gofindthem_amd.engine import Engine
    from test_gpu_multi import _devices
    b = pl.batch("long")
    one, two = _engine(pl.TERMS_ASCII, POS_START, pl.POSITIONS), Engine(devices=_devices())
    try:
        two.build(pl.TERMS_ASCII)
        two.set_programs(_programs(pl.POSITIONS))
        for lead_len in (5, 23):
            buf, off, at = pl.placed("long", "completes", 3, lead_len)
            text = buf[at:]
            csr = one.scan(text, off, fold=True)
            assert_csr_equal(csr, pl.expected_csr("long", POS_START, True))
            assert_csr_equal(two.scan(text, off, fold=True), csr)
            rows = one.process(text, off, fold=True)
            assert np.array_equal(rows, pl.expected_rows("long", pl.POSITIONS, True))
            assert np.array_equal(two.process(text, off, fold=True), rows)
    finally:
        one.close()
        two.close()


# ---- bucket runs of a routed blob --------------------------------------------------------------------------------------------------
def test_routed_buckets_are_scanned_where_they_lie():
    """split_lines_device -> process_device -> route_docs_device, then process_device straight on every bucket's run of the routed
    blob (d_out, d_out_off + bucket_doc[k]): doc_off[0] != 0, any alignment, the neighbouring bucket's text directly in front and
    behind.  The rows are the original rows of the run's documents, bit for bit; the same for the select's one output."""
    lines = pl.batch("short_lines")
    blob = b"".join(lines.docs)
    want = pl.expected_rows("short_lines", pl.POSITIONS, True)
    words, n_cols = _words(pl.POSITIONS), len(pl.expressions(pl.POSITIONS))
    col = {t: i for i, t in enumerate(sorted(set(pl.TERMS_ASCII)))}              # (expression i is the UNIT of keyword i)
    masks = []
    for t in (b"q", b"7", b"tion"):
        m = np.zeros(words, dtype=np.uint32)
        m[col[t] >> 5] = 1 << (col[t] & 31)
        masks.append(m)
    eng = _engine(pl.TERMS_ASCII, POS_START, pl.POSITIONS)
    try:
        text = torch.from_numpy(np.concatenate([np.frombuffer(blob, dtype=np.uint8), np.zeros(64, np.uint8)])).cuda()
        off = eng.split_lines_device(text, len(blob))
        n = off.numel() - 1
        assert n == len(lines.docs)
        bm = torch.zeros((n, words), dtype=torch.int32, device="cuda")
        eng.process_device(text.data_ptr(), off.data_ptr(), n, bm.data_ptr(), fold=True)
        rows = _rows(bm, n)
        assert np.array_equal(rows, want)

        def check_run(out, out_off, first, count, idx, what):
            if not count:
                return
            got = torch.zeros((count, words), dtype=torch.int32, device="cuda")
            eng.process_device(out.data_ptr(), out_off.data_ptr() + 8 * first, count, got.data_ptr(), fold=True)
            assert np.array_equal(_rows(got, count), rows[idx]), (what, _route(eng))

        for mode in ("first", "every"):
            out, out_off, doc_idx, bucket_doc, bucket_byte = eng.route_docs_device(text, off, bm, n_cols, masks, mode=mode, rest=True)
            idx = doc_idx.cpu().numpy()
            assert len(bucket_doc) == 5 and sum(int(bucket_doc[k + 1] > bucket_doc[k]) for k in range(4)) >= 3
            for k in range(4):
                a, b = int(bucket_doc[k]), int(bucket_doc[k + 1])
                for call in range(2):                                # (the second call of a size runs on another route)
                    check_run(out, out_off, a, b - a, idx[a:b], (mode, k, call))
        out, out_off, doc_idx = eng.select_docs_device(text, off, bm, n_cols, want=masks[2], mode="any")
        m = doc_idx.numel()
        assert 0 < m < n
        check_run(out, out_off, 0, m, doc_idx.cpu().numpy(), "select")
    finally:
        eng.close()
