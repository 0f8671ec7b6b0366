"""Hit spans and redaction on the device (csrc/gft_spans.hip): gft_hit_spans_device and gft_redact_spans_device bit-exact against
the reference of spans.py on every fixed case under each production scan kernel, device against host walk on the random batches,
the chain split -> process -> select -> spans with the select's doc_idx as row_idx, the cap protocol into guarded tensors, the
refusals, the profile names, gft_last_nonascii, and the callers Finder.SpansLines / RedactLines.  All comparisons are exact."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before libgft.so is loaded: one HIP runtime)

import spans as S
from gofindthem_amd import _lib
from gofindthem_amd.engine import Engine, GftError, hit_spans_host, pack, witness_terms_host
from gofindthem_amd.finder import EmptyRgxEngine, Finder, FinderError, GpuEngine, PyRegexpEngine

pytestmark = pytest.mark.gpu

GUARD8, GUARD32, GUARD64 = 0xA5, -0x5A5A5A5B, -0x5A5A5A5A5A5A5A5B
KERNELS = ["scan5", "scan3", "dfa"]


class Engines:
    """an engine per (expressions, fold, position mode), built under the scan kernel the environment names when it is first asked for"""

    def __init__(self):
        self.made = {}

    def of(self, c):
        key = (c.exprs, c.fold, c.pos_end)
        if key not in self.made:
            k = S.compiled(c.exprs, c.fold)
            e = Engine()
            e.build(k.terms, pos_end=c.pos_end)
            assert e.terms() == k.terms
            e.set_programs(k.programs, n_extra=k.n_extra)
            self.made[key] = e
        return self.made[key]

    def close(self):
        for e in self.made.values():
            e.close()
        self.made = {}


@pytest.fixture(scope="module")
def engines():
    es = Engines()
    yield es
    es.close()


@pytest.fixture(scope="module")
def eng():
    e = Engine()
    yield e
    e.close()


def resident(lead_and_text, slack=b"", at=0, fill=0):
    """the bytes `at` bytes into an allocation whose other bytes hold `fill`; `slack` lies directly behind them (64 readable bytes
    at least follow the text either way)"""
    data = bytes(lead_and_text) + bytes(slack)
    buf = torch.full((at + len(data) + 64 + 16,), fill, dtype=torch.uint8, device="cuda")
    if data:
        buf[at:at + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    return buf[at:]


class OnDevice:
    def __init__(self, c, fill=0, at=None):
        blob, off = S.packed(c)
        self.c = c
        self.text = resident(blob.tobytes(), c.slack, c.at if at is None else at, fill)
        self.off = torch.from_numpy(off.astype(np.int64)).cuda()
        self.rows = torch.from_numpy(c.rows.view(np.int32).copy()).cuda()
        self.row_idx = torch.from_numpy(c.row_idx.astype(np.int64)).cuda() if c.row_idx is not None else None
        self.n = len(c.docs)


def device_spans(e, d):
    so, a, b, t = e.hit_spans_device(d.text, d.off, d.rows, d.c.want, d.row_idx, fold=d.c.fold)
    return int(a.numel()), so.cpu().tolist(), a.cpu().tolist(), b.cpu().tolist(), t.cpu().tolist()


def host_walk(c):
    k = S.compiled(c.exprs, c.fold)
    wo, we = witness_terms_host(k.programs, k.n_terms, k.n_terms + k.n_extra)
    moff, tid, pos = S.matches(c)
    total, so, a, b, t = hit_spans_host(moff, tid, pos, k.term_len, c.pos_end, wo, we, c.rows, len(k.programs), c.row_idx, c.want)
    return total, so[:len(c.docs) + 1].tolist(), a[:total].tolist(), b[:total].tolist(), t[:total].tolist()


def test_the_cases_are_not_vacuous():
    assert S.assert_not_vacuous()


@pytest.mark.parametrize("kernel", KERNELS)
def test_fixed_cases_under_every_scan_kernel(kernel, monkeypatch):
    monkeypatch.setenv("GFT_SCAN_KERNEL", kernel)                       # (read by gft_build)
    es = Engines()
    try:
        seen = set()
        for c in S.fixed_cases():
            e = es.of(c)
            seen.add(_lib.load().gft_scan_kernel(e._h).decode())
            for fill in (0, 0xFF):
                assert device_spans(e, OnDevice(c, fill)) == S.expected()[c.name], (c.name, fill)
        assert kernel in seen or kernel == "scan5", seen                 # (scan5 asked for but not applicable: as by default)
    finally:
        es.close()


def test_text_at_every_residue(engines):
    for c in S.fixed_cases():
        if c.lead or "tile" in c.name or "abcd" in c.name:
            for at in (0, 1, 3, 8, 15):
                assert device_spans(engines.of(c), OnDevice(c, 0xFF, at)) == S.expected()[c.name], (c.name, at)


def test_random_batches_device_equals_host_walk(engines):
    for c in S.random_cases():
        got = device_spans(engines.of(c), OnDevice(c, 0xFF))
        assert got == host_walk(c), c.name
        assert got == S.expected()[c.name], c.name


def raw_spans(e, d, cap, guard=8, with_len=True, with_term=True, span_off=True):
    """gft_hit_spans_device into guarded tensors -> (total, span_off, start, len, term) on the host, guards included"""
    L = _lib.load()
    c = d.c
    w = np.ascontiguousarray(c.want, dtype=np.uint32) if c.want is not None else None
    so = torch.full((d.n + 1 + guard,), GUARD64, dtype=torch.int64, device="cuda")
    arrs = [torch.full((cap + guard,), GUARD32, dtype=torch.int32, device="cuda") for _ in range(3)]
    total = C.c_uint64(99)
    torch.cuda.synchronize()
    e._check(L.gft_hit_spans_device(e._h, d.text.data_ptr(), d.off.data_ptr(), d.n, _lib.GFT_FOLD_ASCII if c.fold else 0, d.rows.data_ptr(),
                                    d.row_idx.data_ptr() if d.row_idx is not None else None, w.ctypes.data if w is not None else None,
                                    so.data_ptr() if span_off else None, arrs[0].data_ptr(), arrs[1].data_ptr() if with_len else None,
                                    arrs[2].data_ptr() if with_term else None, cap, C.byref(total)))
    return (int(total.value), so.cpu().numpy()) + tuple(a.cpu().numpy() for a in arrs)


def test_cap_protocol_and_guard_words(engines):
    c = next(c for c in S.fixed_cases() if c.name == "mixed documents, rows permuted")
    total, off, start, length, term = S.expected()[c.name]
    e, d = engines.of(c), OnDevice(c)
    for cap in (0, 1, total - 1, total, total + 5):
        t, so, a, b, tm = raw_spans(e, d, cap)
        m = min(cap, total)
        assert t == total and so[:d.n + 1].tolist() == off and (so[d.n + 1:] == GUARD64).all(), cap
        assert a[:m].tolist() == start[:m] and b[:m].tolist() == length[:m] and tm[:m].tolist() == term[:m], cap
        assert (a[m:] == GUARD32).all() and (b[m:] == GUARD32).all() and (tm[m:] == GUARD32).all(), cap
    t, so, a, b, tm = raw_spans(e, d, total, with_len=False, with_term=False, span_off=False)
    assert t == total and a[:total].tolist() == start and (b == GUARD32).all() and (tm == GUARD32).all() and (so == GUARD64).all()
    # count only
    L = _lib.load()
    n = C.c_uint64(0)
    e._check(L.gft_hit_spans_device(e._h, d.text.data_ptr(), d.off.data_ptr(), d.n, 0, d.rows.data_ptr(), d.row_idx.data_ptr(), None, None, None, None, None,
                                    0, C.byref(n)))
    assert n.value == total


def test_profile_names_and_the_scan_state(engines):
    c = next(c for c in S.fixed_cases() if c.name == "mixed documents, identity")
    e, d = engines.of(c), OnDevice(c)
    e.profile(True)
    e.profile_reset()
    try:
        assert device_spans(e, d) == S.expected()[c.name]
        for name in ("span_mark", "span_scan", "span_place"):
            ms, launches = e.profile_read(name)
            assert launches == 2 and ms >= 0, name                      # (the wrapper calls twice: count, then fill)
        so, a, b, t = e.hit_spans_device(d.text, d.off, d.rows)
        text = d.text.clone()
        e.profile_reset()
        e.redact_spans_device(text, d.off, so, a, b, b"#")
        assert e.profile_read("redact_fill")[1] == 1
    finally:
        e.profile(False)
    # it counts as a scan: the engine's CSR is what gft_scan_device leaves for the batch
    L = _lib.load()
    m = _lib.GftMatches()
    e._check(L.gft_scan_device(e._h, d.text.data_ptr(), d.off.data_ptr(), d.n, 0, C.byref(m)))
    moff, tid, pos = S.matches(c)
    assert m.n_matches == len(tid)
    assert device_spans(e, d) == S.expected()[c.name]
    assert e.scan(*pack(["ab", "c"]))[1].size == 3                      # and the handle scans on


def test_last_nonascii_is_as_the_scan_sets_it(engines):
    c = next(c for c in S.fixed_cases() if c.name.startswith("fold-safe Latin-1 text, POS_START"))
    e = engines.of(c)
    L = _lib.load()
    for docs, unsafe in ((["cafe", "abc"], 0), (["café ÿx", "ß"], 0), (["CAFÉ"], 1), (["caf\xc9".encode("latin-1")], 1)):
        d = OnDevice(S.case("x", c.exprs, docs, fold=True))
        for fold in (True, False):
            m = _lib.GftMatches()
            e._check(L.gft_scan_device(e._h, d.text.data_ptr(), d.off.data_ptr(), d.n, 1 if fold else 0, C.byref(m)))
            want = L.gft_last_nonascii(e._h)
            e.scan(*pack(["x"]))                                        # (another verdict in between)
            e.hit_spans_device(d.text, d.off, d.rows, fold=fold)
            assert L.gft_last_nonascii(e._h) == want, (docs, fold)
            assert not fold or want == unsafe, (docs, fold)


def test_refusals_leave_the_handle_usable(engines, eng):
    c = next(c for c in S.fixed_cases() if c.name == "mixed documents, identity")
    e, d = engines.of(c), OnDevice(c)
    L = _lib.load()
    total = C.c_uint64(0)
    so = torch.zeros(d.n + 1, dtype=torch.int64, device="cuda")
    a = torch.zeros(2000, dtype=torch.int32, device="cuda")

    def rc(eh=None, flags=0, text=d.text, rows=d.rows, span_off=so, start=a, cap=2000, n=d.n):
        torch.cuda.synchronize()
        return L.gft_hit_spans_device(eh or e._h, text.data_ptr(), d.off.data_ptr(), n, flags, rows.data_ptr() if rows is not None else None, None, None,
                                      span_off.data_ptr() if span_off is not None else None, start.data_ptr() if start is not None else None, None, None,
                                      cap, C.byref(total))

    def still_good():
        assert device_spans(e, d) == S.expected()[c.name]
    assert rc() == 0 and total.value == S.expected()[c.name][0]
    for flags in (_lib.GFT_SCAN_UNIQUE, _lib.GFT_POS_RUNES, 8):
        assert rc(flags=flags) == _lib.GFT_E_INVALID and total.value == 0
        still_good()
    assert rc(start=None) == _lib.GFT_E_INVALID                         # a cap without its array
    assert rc(rows=None) == _lib.GFT_E_INVALID
    assert rc(span_off=d.off) == _lib.GFT_E_INVALID                     # outputs that are inputs
    assert rc(start=d.rows, cap=3) == _lib.GFT_E_INVALID
    assert rc(span_off=d.text) == _lib.GFT_E_INVALID
    both = torch.zeros(4 * (d.n + 1), dtype=torch.int32, device="cuda")
    assert rc(span_off=both.view(torch.int64), start=both, cap=4) == _lib.GFT_E_INVALID     # outputs that overlap each other
    still_good()
    # no dictionary, no programs
    assert rc(eh=eng._h) == _lib.GFT_E_NOT_BUILT
    eng.build([b"a"])
    assert rc(eh=eng._h) == _lib.GFT_E_NOT_BUILT
    eng.set_programs([[1 << 28]])
    assert rc(eh=eng._h, rows=torch.full((d.n,), -1, dtype=torch.int32, device="cuda")) == 0 and total.value == S.matches(c)[1].tolist().count(0)
    eng.set_programs([])                                                # no expressions: no span
    assert rc(eh=eng._h, rows=None) == 0 and total.value == 0 and not so.cpu().numpy().any()
    assert rc(n=0) == 0 and total.value == 0                            # no documents
    # between _begin and _end only after _complete
    bm = torch.zeros(d.n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for _ in range(3):                                                  # (an engine's first batches complete inside _begin)
        e._check(L.gft_process_device_begin(e._h, d.text.data_ptr(), d.off.data_ptr(), d.n, 0, None, bm.data_ptr()))
        if rc() == _lib.GFT_E_INVALID:
            assert rc() == _lib.GFT_E_INVALID
            assert L.gft_redact_spans_device(e._h, d.text.data_ptr(), d.off.data_ptr(), d.n, so.data_ptr(), a.data_ptr(), a.data_ptr(), 42) == _lib.GFT_E_INVALID
            e._check(L.gft_process_device_complete(e._h))
            assert rc() == 0
        e._check(L.gft_process_device_end(e._h))
    still_good()


def test_the_witness_table_follows_the_programs(eng):
    """compiled lazily after gft_set_programs, dropped by gft_set_programs and gft_build"""
    text = resident(b"ab ba")
    off = torch.tensor([0, 2, 5], dtype=torch.int64, device="cuda")
    rows = torch.tensor([1, 1], dtype=torch.int32, device="cuda")
    eng.build([b"a", b"b"])
    UNIT, AND, NOT = 1 << 28, 2 << 28, 4 << 28
    for prog, terms in (([UNIT | 0, UNIT | 1, AND], [0, 1, 1, 0]), ([UNIT | 0, UNIT | 1, NOT, AND], [0, 0]), ([UNIT | 1], [1, 1])):
        eng.set_programs([prog])
        assert eng.hit_spans_device(text, off, rows)[3].cpu().tolist() == terms
        assert eng.hit_spans_device(text, off, rows)[3].cpu().tolist() == terms
    eng.build([b"b", b"c"])
    eng.set_programs([[UNIT | 0]])
    assert eng.hit_spans_device(text, off, rows)[3].cpu().tolist() == [0, 0]


class FillOnDevice:
    def __init__(self, f, at=0):
        self.f = f
        buf = torch.full((at + f.blob.size + 32,), GUARD8, dtype=torch.uint8, device="cuda")
        buf[at:at + f.blob.size] = torch.from_numpy(f.blob.copy()).cuda()
        self.buf, self.at = buf, at
        self.text = buf[at:]
        self.off = torch.from_numpy(f.doc_off.astype(np.int64)).cuda()
        self.span_off = torch.from_numpy(f.span_off.astype(np.int64)).cuda()
        self.start = torch.from_numpy(f.start.view(np.int32).copy()).cuda()
        self.length = torch.from_numpy(f.length.view(np.int32).copy()).cuda()

    def expect(self, body):
        return bytes([GUARD8]) * self.at + body + bytes([GUARD8]) * 32


def test_redaction(eng):
    for f in S.fill_cases():
        for at in (0, 1, 7):
            d = FillOnDevice(f, at)
            if f.ok:
                eng.redact_spans_device(d.text, d.off, d.span_off, d.start, d.length, f.mask)
                assert d.buf.cpu().numpy().tobytes() == d.expect(S.redact_reference(f)), (f.name, at)
            else:
                with pytest.raises(GftError) as ei:
                    eng.redact_spans_device(d.text, d.off, d.span_off, d.start, d.length, f.mask)
                assert ei.value.code == _lib.GFT_E_INVALID
                assert d.buf.cpu().numpy().tobytes() == d.expect(f.blob.tobytes()), (f.name, at)     # nothing was written
    # the handle is usable after the refusals; a mask beyond a byte; no documents
    d = FillOnDevice(S.fill_cases()[0])
    L = _lib.load()
    args = (eng._h, d.text.data_ptr(), d.off.data_ptr(), len(d.f.doc_off) - 1, d.span_off.data_ptr(), d.start.data_ptr(), d.length.data_ptr())
    assert L.gft_redact_spans_device(*args, 256) == _lib.GFT_E_INVALID
    assert L.gft_redact_spans_device(eng._h, None, None, 0, None, None, None, 42) == 0
    assert d.buf.cpu().numpy().tobytes() == d.expect(d.f.blob.tobytes())
    assert L.gft_redact_spans_device(*args, d.f.mask) == 0
    assert d.buf.cpu().numpy().tobytes() == d.expect(S.redact_reference(d.f))


def test_spans_then_redaction_on_the_device(engines):
    for c in S.fixed_cases():
        if not ("abcd" in c.name or "Latin" in c.name or "mixed documents, identity" == c.name):
            continue
        e, d = engines.of(c), OnDevice(c, 0x41)
        so, a, b, t = e.hit_spans_device(d.text, d.off, d.rows, c.want, d.row_idx, fold=c.fold)
        before = d.text.cpu().numpy().copy()
        e.redact_spans_device(d.text, d.off, so, a, b, b"#")
        blob, off = S.packed(c)
        total, span_off, start, length, _ = S.expected()[c.name]
        f = S.FillCase(c.name, before, off, np.asarray(span_off, dtype=np.uint64), np.asarray(start, dtype=np.uint32), np.asarray(length, dtype=np.uint32),
                       ord("#"), True)
        assert d.text.cpu().numpy().tobytes() == S.redact_reference(f), c.name


LOG = [b"GET /index.html 200", b"POST /login 401 bad password for root", b"GET /admin 403", b"kernel: oom-killer invoked", b"",
       b"POST /login 200 root", b"GET /health 200", b"sshd: Failed password for root from 10.0.0.7", b"cron: job done"] * 40
LOG_EXPRS = ['"password" and "root"', '"403" or "oom"', '"GET" and not "200"', 'inord("POST" and "login")']


def test_chain_split_process_select_spans(eng):
    """the lines that hit are gathered by the select; their spans are explained against the rows of the batch they came from"""
    k = S.compiled(tuple(LOG_EXPRS), False)
    eng.build(k.terms)
    eng.set_programs(k.programs)
    data = b"".join(ln + b"\n" for ln in LOG)
    buf = resident(data)
    off = eng.split_lines_device(buf, len(data))
    n = int(off.numel()) - 1
    bm = torch.zeros((n, 1), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng.process_device(buf.data_ptr(), off.data_ptr(), n, bm.data_ptr())
    want = S.want_of(4, [0, 1])
    out, out_off, doc_idx = eng.select_docs_device(buf, off, bm, 4, want)
    got = eng.hit_spans_device(out, out_off, bm, want, doc_idx)
    # the reference on the selected lines, rows from the oracle
    lines = [ln + b"\n" for ln in LOG]
    rows = S.true_rows(tuple(LOG_EXPRS), tuple(lines), False)
    assert np.array_equal(bm.cpu().numpy().view(np.uint32) & 15, rows & 15)
    idx = [i for i in range(n) if int(rows[i, 0]) & 3]
    assert doc_idx.cpu().tolist() == idx
    c = S.case("chain", LOG_EXPRS, [lines[i] for i in idx], rows=rows, row_idx=idx, want=want)
    total, span_off, start, length, term = S.reference(c)
    assert total > 0 and (got[0].cpu().tolist(), got[1].cpu().tolist(), got[2].cpu().tolist(), got[3].cpu().tolist()) == (span_off, start, length, term)
    # ... and the same spans from the unselected batch, document by document
    full = eng.hit_spans_device(buf, off, bm, want)
    fo, fs = full[0].cpu().tolist(), full[1].cpu().tolist()
    assert [fs[fo[i]:fo[i + 1]] for i in idx] == [start[span_off[j]:span_off[j + 1]] for j in range(len(idx))]


def finder_reference(exprs, lines, want_cols=None, mask=ord("*")):
    """(idx, spans, masked bytes) of the contract over lines that are already as the finder scans them"""
    c = S.case("finder", exprs, lines)
    if want_cols is not None:
        c = c._replace(want=S.want_of(len(exprs), want_cols))
    total, span_off, start, length, term = S.reference(c)
    k = S.compiled(tuple(exprs), False)
    w = (1 << len(exprs)) - 1 if want_cols is None else sum(1 << i for i in want_cols)
    idx = [d for d in range(len(lines)) if int(c.rows[d, 0]) & w]
    spans = [[(start[s], start[s] + length[s], k.terms[term[s]]) for s in range(span_off[d], span_off[d + 1])] for d in idx]
    blob, off = S.packed(c)
    f = S.FillCase("finder", blob, off, np.asarray(span_off, dtype=np.uint64), np.asarray(start, dtype=np.uint32), np.asarray(length, dtype=np.uint32),
                   mask, True)
    return idx, spans, S.redact_reference(f), (span_off, start, length)


@pytest.mark.parametrize("kind", ["ascii", "latin-1, fold-safe", "an upper-case non-ASCII letter"])
def test_finder_spans_lines_and_redact_lines(kind):
    lines = [ln + b"\n" for ln in LOG[:27]]
    lowered = kind == "an upper-case non-ASCII letter"
    if kind != "ascii":
        lines[2] = "GET /café 403 ÿ\n".encode()
    if lowered:
        lines[3] = "KERNEL: OOM-killer \u0130nvoked by CAF\u00c9\n".encode()     # (U+0130 shrinks under ToLower: the offsets move)
    exprs = LOG_EXPRS + ['"café" or "ÿ"']
    data = b"".join(lines)
    L = _lib.load()

    def to_lower(b):
        out = np.zeros(3 * len(b) + 1, dtype=np.uint8)
        n = C.c_uint64(0)
        assert L.gft_to_lower(b, len(b), out.ctypes.data, out.size, C.byref(n)) == 0
        return out[:n.value].tobytes()
    # what a case-insensitive finder scans: strings.ToLower of every line, against keywords the parser lower-cased
    scanned = [to_lower(ln) for ln in lines]
    low_exprs = [e.replace("GET", "get").replace("POST", "post") for e in exprs]
    f = Finder(GpuEngine.__new__(GpuEngine), EmptyRgxEngine(), False)
    try:
        f.AddExpressions(exprs)
        idx, spans, low = f.SpansLines(data)
        masked, low2 = f.RedactLines(data)
        assert low == low2 == lowered
        ref_idx, ref_spans, ref_masked, (span_off, start, length) = finder_reference(low_exprs, scanned)
        assert idx.tolist() == ref_idx and spans == ref_spans and any(spans)
        if lowered:
            assert masked == ref_masked and len(masked) != len(data)
        else:
            # the caller's own bytes with the masks in them: the upper-case letters outside the spans stay
            own, o = bytearray(data), 0
            for d, ln in enumerate(lines):
                for s in range(span_off[d], span_off[d + 1]):
                    own[o + start[s]:o + start[s] + length[s]] = b"*" * length[s]
                o += len(ln)
            assert masked == bytes(own) and masked != ref_masked
        # one column, another mask byte
        w = f.want_mask([1])
        idx1, spans1, _ = f.SpansLines(data, w)
        r1 = finder_reference(low_exprs, scanned, [1], ord("#"))
        assert idx1.tolist() == r1[0] and spans1 == r1[1]
        assert to_lower(f.RedactLines(data, w, b"#")[0]) == r1[2]
    finally:
        f.close()


def test_finder_spans_need_the_device_route():
    f = Finder(GpuEngine.__new__(GpuEngine), PyRegexpEngine(), True)
    try:
        f.AddExpression('"a" and r"b+"')
        with pytest.raises(FinderError) as ei:
            f.SpansLines(b"a bb\n")
        assert ei.value.code == _lib.GFT_E_UNSUPPORTED
    finally:
        f.close()
