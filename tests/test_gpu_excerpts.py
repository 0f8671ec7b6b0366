"""Excerpts on the device (csrc/gft_excerpt.hip, the copy pass of csrc/gft_select.hip): gft_excerpt_spans_device bit for bit against
the reference of excerpts.py on every fixed case -- each twice, with the lead bytes, the slack and the allocations round every
output filled with 0x00 and with 0xBF, a continuation byte -- and against the host walk on the random batches; the text at five
residues of the 16-byte grid; the cap protocol into guarded tensors; every output NULL on its own; the refusals, which leave every
output untouched and the handle usable; the chains split -> process -> spans -> excerpt -> redact and process -> select / route
-> spans with row_idx -> excerpt against slicing on the host; Finder.ExcerptLines over a batch that is lowered; the profile names
and gft_last_nonascii.  All comparisons are exact."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before libgft.so is loaded: one HIP runtime)

import excerpts as X
from gofindthem_amd import _lib
from gofindthem_amd.engine import Engine, excerpt_shape, excerpt_spans_host
from gofindthem_amd.finder import EmptyRgxEngine, Finder, GpuEngine

pytestmark = pytest.mark.gpu

TILE, TRIP = excerpt_shape() if hasattr(_lib.load(), "gft_debug_excerpt_shape") else (256, 1024)
G = 8                                                               # guard entries on either side of every output
NAMES = ("out", "exc_off", "exc_doc", "exc_start", "exc_span_off", "span_rel", "doc_exc_off")
DTYPES = {"out": torch.uint8, "exc_off": torch.int64, "exc_doc": torch.int64, "exc_start": torch.int32, "exc_span_off": torch.int64,
          "span_rel": torch.int32, "doc_exc_off": torch.int64}


@pytest.fixture(scope="module")
def eng():
    e = Engine()
    yield e
    e.close()


_REF = {}


def reference(case):
    if case.name not in _REF:
        _REF[case.name] = X.expected(case)
    return _REF[case.name]


class OnDevice:
    """a case on the device: the text `at` bytes into an allocation whose every other byte -- in front, the lead, the 64 bytes of
    slack -- holds `fill`"""

    def __init__(self, case, fill=0x00, at=0):
        self.case = case
        self.blob, self.off, self.so, self.st, self.ln = case.arrays(fill)
        buf = torch.full((at + self.blob.size + 64,), fill, dtype=torch.uint8, device="cuda")
        if self.blob.size:
            buf[at:at + self.blob.size] = torch.from_numpy(self.blob.copy()).cuda()
        self.text = buf[at:]
        self.n = len(case.docs)
        self.d_off = torch.from_numpy(self.off.astype(np.int64)).cuda()
        self.d_so = torch.from_numpy(self.so.astype(np.int64)).cuda()
        self.d_st = torch.from_numpy(self.st.view(np.int32).copy()).cuda()
        self.d_ln = torch.from_numpy(self.ln.view(np.int32).copy()).cuda()
        self.fill = fill

    def call(self, e, outs=None, cap_bytes=0, cap_exc=0, flags=None, before=None, after=None, handle=None):
        """the raw call -> (rc, n_exc, total); outs: name -> tensor"""
        outs = outs or {}
        m, total = C.c_uint64(0), C.c_uint64(0)
        p = {k: (outs[k].data_ptr() if outs.get(k) is not None else None) for k in NAMES}
        c = self.case
        torch.cuda.synchronize()
        rc = _lib.load().gft_excerpt_spans_device(
            handle or e._h, self.text.data_ptr(), self.d_off.data_ptr(), self.n, self.d_so.data_ptr(),
            self.d_st.data_ptr() if self.st.size else None, self.d_ln.data_ptr() if self.ln.size else None,
            c.before if before is None else before, c.after if after is None else after,
            (1 if c.runes else 0) if flags is None else flags, p["out"], cap_bytes, p["exc_off"], p["exc_doc"], p["exc_start"], p["exc_span_off"],
            cap_exc, p["span_rel"], p["doc_exc_off"], C.byref(m), C.byref(total))
        return rc, int(m.value), int(total.value)

    def sizes(self, m, total):
        return {"out": total, "exc_off": m + 1, "exc_doc": m, "exc_start": m, "exc_span_off": m + 1, "span_rel": self.st.size, "doc_exc_off": self.n + 1}

    def guarded(self, sizes, shift=0):
        """name -> (allocation filled with the pattern, the view the call gets): G entries of guard on either side; the byte output
        `shift` bytes further into the 16-byte grid"""
        full, view = {}, {}
        pat = 0xBF if self.fill else 0x5A
        for k, n in sizes.items():
            extra = shift if k == "out" else 0
            t = torch.empty(n + 2 * G + extra, dtype=DTYPES[k], device="cuda")
            t.view(torch.uint8).fill_(pat)
            full[k], view[k] = t, t[G + extra:G + extra + n]
        return full, view, pat

    def run(self, e, cap_bytes=None, cap_exc=None, omit=(), shift=0):
        """count, then fill guarded tensors -> a dict like the reference's, arrays cut to what the caps allow; the guards checked"""
        rc, m, total = self.call(e)
        assert rc == 0, _lib.load().gft_last_error(e._h)
        cb = total if cap_bytes is None else cap_bytes
        ce = m if cap_exc is None else cap_exc
        sizes = self.sizes(min(m, ce), min(total, cb))
        sizes["exc_off"] = sizes["exc_span_off"] = min(m, ce) + 1
        full, view, pat = self.guarded(sizes, shift)
        for k in omit:
            view[k] = None
        rc, m2, total2 = self.call(e, view, cb, ce)
        assert rc == 0 and (m2, total2) == (m, total), _lib.load().gft_last_error(e._h)
        got = {"n_exc": m, "total": total}
        for k in NAMES:
            raw = full[k].view(torch.uint8).cpu().numpy()
            item = full[k].element_size()
            extra = shift if k == "out" else 0
            lo, hi = (G + extra) * item, (G + extra + sizes[k]) * item
            assert (raw[:lo] == pat).all() and (raw[hi:] == pat).all(), "%s: a store outside the output" % k
            if k in omit:
                assert (raw == pat).all(), "%s: not passed, yet written" % k
            got[k] = None if k in omit else view[k].cpu().numpy()
        if got["out"] is not None:
            got["out"] = got["out"].tobytes()
        return got


def assert_same(got, want, what):
    diff = X.same(got, want)
    assert diff is None, "%s: %s" % (what, diff)


FIXED = X.fixed_cases(TILE, TRIP)
RESIDUES = (0, 1, 3, 8, 15)


@pytest.mark.parametrize("i", range(len(FIXED)), ids=[c.name for c in FIXED])
def test_fixed_case(eng, i):
    case = FIXED[i]
    want = reference(case)
    for fill in (0x00, 0xBF):
        at = RESIDUES[(i + (fill != 0)) % len(RESIDUES)]
        assert_same(OnDevice(case, fill, at).run(eng, shift=at % 7), want, "%s, fill %#x, text at +%d" % (case.name, fill, at))


@pytest.mark.parametrize("at", RESIDUES)
def test_placement(eng, at):
    """the text at every residue, behind lead bytes (doc_off[0] != 0), the output at every residue too"""
    for name in ("rune snap 2/3", "one excerpt past the copy's tile", "doc_off[0] != 0"):
        case = next(c for c in FIXED if c.name == name)
        case = case.but(case.name + ", lead", lead=case.lead + 5)
        want = X.expected(case)
        for fill in (0x00, 0xBF):
            assert_same(OnDevice(case, fill, at).run(eng, shift=(at * 5) % 16), want, "%s, fill %#x, at +%d" % (name, fill, at))


def test_random_batches_against_the_host_walk(eng):
    for case in X.random_cases():
        d = OnDevice(case, 0xBF, case.lead % 3)
        r = excerpt_spans_host(d.blob, d.off, d.so, d.st, d.ln, case.before, case.after, case.runes)
        m, total = r["n_exc"], r["total"]
        want = {"n_exc": m, "total": total, "out": (r["out"][:total].tobytes() if r["out"] is not None else b"")}
        for k in X.ARRAYS:
            want[k] = [] if r[k] is None else r[k].tolist()
        assert_same(d.run(eng), want, case.name)


def test_cap_protocol(eng):
    case = next(c for c in FIXED if c.name == "one excerpt past the copy's tile")
    want = reference(case)
    m, total = want["n_exc"], want["total"]
    d = OnDevice(case, 0xBF, 3)
    assert d.call(eng) == (0, m, total)                              # count only
    assert_same(d.run(eng, total, m), want, "exact caps")
    got = d.run(eng, cap_exc=m - 1)                                  # one entry short: nothing at or past the cap (run checks the guards)
    assert got["exc_off"].tolist() == want["exc_off"][:m] and got["exc_span_off"].tolist() == want["exc_span_off"][:m]
    assert got["exc_doc"].tolist() == want["exc_doc"][:m - 1] and got["exc_start"].tolist() == want["exc_start"][:m - 1]
    assert got["span_rel"].tolist() == want["span_rel"] and got["doc_exc_off"].tolist() == want["doc_exc_off"] and got["out"] == want["out"]
    capb = want["exc_off"][2] + 1000                                 # in the middle of the long excerpt
    for cb in (capb, capb + 7, want["exc_off"][2], 1):
        got = d.run(eng, cap_bytes=cb, shift=5)
        assert got["out"] == want["out"][:cb] and got["exc_off"].tolist() == want["exc_off"], cb


@pytest.mark.parametrize("name", NAMES)
def test_every_output_null_on_its_own(eng, name):
    case = next(c for c in FIXED if c.name == "one excerpt past the copy's tile")
    want = reference(case)
    got = OnDevice(case).run(eng, omit=(name,), cap_bytes=0 if name == "out" else None)
    for k in NAMES:
        if k != name:
            assert (got[k] == want[k]) if k == "out" else (got[k].tolist() == want[k]), k


def test_refusals_write_nothing_and_leave_the_handle_usable(eng):
    L = _lib.load()
    base = X.runs_case("refusals", [TILE, 40])
    n = TILE + 40
    good = reference(base)
    order, past = X.refusal_spans(base, n - 5)                      # one pair of ends that descend, in the last tile
    assert n - 5 >= TILE
    for bad in (base.but("order", spans=[order]), base.but("past the end", spans=[past])):
        d = OnDevice(bad, 0xBF)
        full, view, pat = d.guarded(d.sizes(good["n_exc"], good["total"]))
        rc, m, total = d.call(eng, view, good["total"], good["n_exc"])
        assert rc == _lib.GFT_E_INVALID and (m, total) == (0, 0), bad.name
        for k in NAMES:
            assert (full[k].view(torch.uint8).cpu().numpy() == pat).all(), "%s: %s was written" % (bad.name, k)
        assert_same(OnDevice(base).run(eng), good, "after the refusal of " + bad.name)
    d = OnDevice(base)
    assert d.call(eng, flags=2)[0] == _lib.GFT_E_INVALID and d.call(eng, flags=0x80000001)[0] == _lib.GFT_E_INVALID
    full, view, _ = d.guarded(d.sizes(good["n_exc"], good["total"]))
    assert d.call(eng, {"out": view["out"]}, 0, 0)[0] == 0          # (an output without its cap is simply not written)
    assert d.call(eng, {}, 5, 0)[0] == _lib.GFT_E_INVALID           # cap_bytes without an output
    # outputs that are inputs, outputs that overlap each other
    assert d.call(eng, {"span_rel": d.d_st})[0] == _lib.GFT_E_INVALID
    assert d.call(eng, {"out": d.text[4:]}, 8, 0)[0] == _lib.GFT_E_INVALID
    assert d.call(eng, {"doc_exc_off": d.d_off})[0] == _lib.GFT_E_INVALID
    both = torch.zeros(8, dtype=torch.int64, device="cuda")
    assert d.call(eng, {"exc_off": both, "exc_doc": both[1:]}, 0, 2)[0] == _lib.GFT_E_INVALID
    # offsets that descend
    d2 = OnDevice(X.Case("two", [b"abcdef", b"ghij"], [[(1, 1)], [(1, 1)]], 1, 1))
    d2.d_off = torch.tensor([0, 12, 10], dtype=torch.int64, device="cuda")
    assert d2.call(eng)[0] == _lib.GFT_E_INVALID
    d2 = OnDevice(X.Case("two", [b"abcdef", b"ghij", b"k"], [[(1, 1)], [(1, 1)], []], 1, 1))
    d2.d_so = torch.tensor([0, 2, 1, 2], dtype=torch.int64, device="cuda")
    assert d2.call(eng)[0] == _lib.GFT_E_INVALID and b"span offsets descend" in L.gft_last_error(eng._h)
    # both at once, in different documents: one message, always the same (a control word a condition)
    d2.d_off = torch.tensor([3, 2, 6, 11], dtype=torch.int64, device="cuda")
    for _ in range(3):
        assert d2.call(eng)[0] == _lib.GFT_E_INVALID and b"span offsets descend" in L.gft_last_error(eng._h)
    # a handle over several devices
    multi = Engine(devices=[0, 0])
    try:
        assert d.call(eng, handle=multi._h)[0] == _lib.GFT_E_UNSUPPORTED
    finally:
        multi.close()
    # no documents
    eo = torch.full((2,), 7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert L.gft_excerpt_spans_device(eng._h, None, None, 0, None, None, None, 3, 3, 1, None, 0, eo.data_ptr(), None, None, None, 0, None, None,
                                      None, None) == 0
    assert eo.cpu().tolist() == [0, 7]
    # ... whose offsets are not read when given: exc_span_off[0] is 0, as on the host
    nine = torch.full((1,), 9, dtype=torch.int64, device="cuda")
    eso = torch.full((2,), 7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert L.gft_excerpt_spans_device(eng._h, None, nine.data_ptr(), 0, nine.data_ptr(), None, None, 3, 3, 1, None, 0, None, None, None,
                                      eso.data_ptr(), 0, None, None, None, None) == 0
    assert eso.cpu().tolist() == [0, 7]
    h, h9 = np.full(2, 7, np.uint64), np.full(1, 9, np.uint64)
    assert L.gft_debug_excerpt_spans(None, None, 0, h9.ctypes.data, None, None, 3, 3, 1, None, 0, None, None, None,
                                     h.ctypes.data, 0, None, None, None, None) == 0 and h.tolist() == [0, 7]
    assert_same(OnDevice(base).run(eng), good, "after every refusal")


def test_profile_names_and_last_nonascii(eng):
    L = _lib.load()
    case = next(c for c in FIXED if c.name == "a run crosses a tile border")
    d = OnDevice(case)
    eng.build([b"ab"])
    m = _lib.GftMatches()
    text = torch.zeros(80, dtype=torch.uint8, device="cuda")
    text[:5] = torch.tensor(list("CAFÉ".encode()), dtype=torch.uint8)
    off = torch.tensor([0, 5], dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    eng._check(L.gft_scan_device(eng._h, text.data_ptr(), off.data_ptr(), 1, 1, C.byref(m)))
    before = L.gft_last_nonascii(eng._h)
    assert before == 1
    eng.profile(True)
    eng.profile_reset()
    got = d.run(eng)
    assert_same(got, reference(case), case.name)
    for name in ("excerpt_window", "excerpt_smin", "excerpt_scan", "excerpt_place"):
        assert eng.profile_read(name)[1] == 2, name                 # (run calls twice: count, fill)
    assert eng.profile_read("excerpt_copy")[1] == 1 and eng.profile_read("select_copy")[1] == 0
    eng.profile(False)
    assert L.gft_last_nonascii(eng._h) == before


# ---- the chains ------------------------------------------------------------------------------------------------------------------
LOG = [b"GET /index.html 200", b"POST /login 401 bad password for root", b"GET /admin 403", b"kernel: oom-killer invoked", b"",
       b"POST /login 200 root", b"GET /health 200", b"sshd: Failed password for root from 10.0.0.7", b"cron: job done"] * 3
LOG_EXPRS = ['"password" and "root"', '"403" or "oom"', '"GET" and not "200"', 'inord("POST" and "login")', '"café" or "ÿ"']


@pytest.fixture(scope="module")
def finder():
    f = Finder(GpuEngine.__new__(GpuEngine), EmptyRgxEngine(), False)
    f.AddExpressions(LOG_EXPRS)
    yield f
    f.close()


def resident(data):
    buf = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda")
    buf[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    return buf


def as_case(name, docs, so, st, ln, before, after, runes=True):
    so, st, ln = (t.cpu().numpy().astype(np.int64) for t in (so, st, ln))
    so = so - so[0]
    return X.Case(name, docs, [list(zip(st[so[d]:so[d + 1]].tolist(), ln[so[d]:so[d + 1]].tolist())) for d in range(len(docs))], before, after, runes)


def tensors_as_result(t):
    out, exc_off, exc_doc, exc_start, exc_span_off, span_rel, doc_exc_off = t[:7]
    r = {"n_exc": int(exc_doc.numel()), "total": int(out.numel()), "out": out.cpu().numpy().tobytes()}
    for k, v in zip(X.ARRAYS, (exc_off, exc_doc, exc_start, exc_span_off, span_rel, doc_exc_off)):
        r[k] = v.cpu().numpy()
    return r


def test_chain_split_process_spans_excerpt_redact(finder):
    lines = [ln + b"\n" for ln in LOG]
    data = b"".join(lines)
    buf = resident(data)
    off, bm = finder.ProcessLinesDevice(buf, len(data))
    so, st, ln, tm, low = finder.SpansDevice(buf, off, bm)
    assert not low and int(st.numel()) > 20
    t = finder.ExcerptsDevice(buf, off, so, st, ln, low, False, 6, 4)
    case = as_case("log", lines, so, st, ln, 6, 4)
    want = X.expected(case)
    assert_same(tensors_as_result(t), want, "split -> process -> spans -> excerpt")
    assert t[7] is False and want["n_exc"] > 10
    # ... and (out, exc_off, exc_span_off, span_rel, span_len) is what the redaction takes
    out, exc_off, _, _, exc_span_off, span_rel = t[:6]
    masked = out.clone()
    L = _lib.load()
    torch.cuda.synchronize()
    rc = L.gft_redact_spans_device(finder.engine_handle(), masked.data_ptr(), exc_off.data_ptr(), want["n_exc"], exc_span_off.data_ptr(),
                                   span_rel.data_ptr(), ln.data_ptr(), ord("#"))
    assert rc == 0
    ref = bytearray(want["out"])
    flat = [x for s in case.spans for x in s]
    for k in range(want["n_exc"]):
        for j in range(want["exc_span_off"][k], want["exc_span_off"][k + 1]):
            a = want["exc_off"][k] + want["span_rel"][j]
            ref[a:a + flat[j][1]] = b"#" * flat[j][1]
    assert masked.cpu().numpy().tobytes() == bytes(ref) and b"#" in ref and bytes(ref) != want["out"]


def test_chain_select_and_route_with_row_idx(finder):
    lines = [ln + b"\n" for ln in LOG]
    data = b"".join(lines)
    want_mask = finder.want_mask([0, 1])
    out, out_off, doc_idx, off, bm = finder.SelectLinesDevice(resident(data), len(data), want_mask)
    so, st, ln, tm, low = finder.SpansDevice(out, out_off, bm, want_mask, row_idx=doc_idx)
    picked = [lines[i] for i in doc_idx.cpu().tolist()]
    t = finder.ExcerptsDevice(out, out_off, so, st, ln, low, False, 5, 5)
    assert_same(tensors_as_result(t), X.expected(as_case("selected", picked, so, st, ln, 5, 5)), "process -> select -> spans -> excerpt")
    assert len(picked) >= 9 and int(t[2].numel()) >= len(picked)
    # a route's bucket run as the batch: doc_off[0] != 0
    out, out_off, doc_idx, bucket_doc, bucket_byte, off, bm = finder.RouteLinesDevice(resident(data), len(data), [[0], [1]])
    b0, b1 = int(bucket_doc[1]), int(bucket_doc[2])
    assert b1 > b0 > 0 and int(bucket_byte[1]) > 0
    run_off, run_idx = out_off[b0:b1 + 1].contiguous(), doc_idx[b0:b1].contiguous()
    so, st, ln, tm, low = finder.SpansDevice(out, run_off, bm, finder.want_mask([1]), row_idx=run_idx)
    picked = [lines[i] for i in run_idx.cpu().tolist()]
    t = finder.ExcerptsDevice(out, run_off, so, st, ln, low, False, 3, 7)
    assert_same(tensors_as_result(t), X.expected(as_case("bucket", picked, so, st, ln, 3, 7)), "a route's bucket run")
    assert int(t[2].numel()) >= len(picked)


def test_excerpt_lines_of_a_lowered_batch(finder):
    lines = [ln + b"\n" for ln in LOG]
    lines[2] = "GET /café 403 ÿ\n".encode()
    lines[3] = "KERNEL: OOM-killer İnvoked by CAFÉ\n".encode()        # U+0130 shrinks: what follows moves to the left
    lines[6] = "Ⱥ grows, then a password for root ⱥⱥⱥ\n".encode()     # U+023A grows: what follows moves to the right
    lines[7] = b"\x80 oom behind a lone continuation byte 403\n"       # an invalid byte becomes three
    data = b"".join(lines)
    sidx, sspans, slow = finder.SpansLines(data, source=True)
    idx, exc, low = finder.ExcerptLines(data, before=9, after=9, source=True)
    assert low and slow and idx.tolist() == sidx.tolist() and {2, 3, 6, 7} <= set(idx.tolist())
    for d, per_line, sp in zip(idx.tolist(), exc, sspans):
        line = lines[d]
        assert sum(len(h) for _, _, h in per_line) == len(sp)
        hits = []
        for start, text, h in per_line:
            assert line[start:start + len(text)] == text, (d, start)                 # a substring of the caller's line ...
            for cut in (start, start + len(text)):                                     # ... cut on rune borders
                assert cut in (0, len(line)) or (line[cut] & 0xC0) != 0x80, (d, cut)
            hits += [(start + a, start + b, kw) for a, b, kw in h]
        assert hits == sp, d
        want = X.expected(X.Case("line", [line], [[(a, b - a) for a, b, _ in sp]], 9, 9))
        assert [(s, t) for s, t, _ in per_line] == list(zip(want["exc_start"], [want["out"][a:b] for a, b in zip(want["exc_off"], want["exc_off"][1:])]))
    # source=False: the excerpts are cut from the lines' lower-case form
    lidx, lspans, llow = finder.SpansLines(data)
    idx2, exc2, low2 = finder.ExcerptLines(data, before=9, after=9, source=False)
    assert low2 and llow and idx2.tolist() == lidx.tolist()
    for d, per_line, sp in zip(idx2.tolist(), exc2, lspans):
        hits = []
        for start, text, h in per_line:
            for a, b, kw in h:
                assert text[a:b] == kw, (d, a, b, kw)                                  # the lowered text shows the keyword itself
            hits += [(start + a, start + b, kw) for a, b, kw in h]
        assert hits == sp, d
    assert exc2 != exc
    # an ASCII batch: both forms agree and nothing is lowered
    data = b"".join(ln + b"\n" for ln in LOG)
    a, b = finder.ExcerptLines(data, source=True), finder.ExcerptLines(data, source=False)
    assert a[2] is False and b[2] is False and a[0].tolist() == b[0].tolist() and a[1] == b[1] and any(a[1])
