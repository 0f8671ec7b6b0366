"""Highlight on the device (csrc/gft_mark.hip, the run passes of csrc/gft_excerpt.hip): gft_mark_spans_device bit for bit against
the reference of mark.py on every fixed case -- each twice, with the lead bytes, the slack and the allocations round every output
filled with 0x00 and with a byte of the marker -- and on the random batches; the text at five residues of the 16-byte grid, the
output shifted by 1, 7 and 15 bytes; the span counts round the borders of the run passes' walk; the cap protocol into guarded
tensors; every output NULL on its own; the refusals, which leave every output untouched and the handle usable; the chains
split -> process -> spans -> mark, select / route -> spans with row_idx -> mark, excerpt -> mark, mark -> redact, mark twice;
Finder.HighlightLines over a batch that is lowered and ExcerptLines(mark=); the profile names and gft_last_nonascii.  All
comparisons are exact."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before libgft.so is loaded: one HIP runtime)

import mark as M
from gofindthem_amd import _lib
from gofindthem_amd.engine import Engine, mark_shape
from gofindthem_amd.finder import EmptyRgxEngine, Finder, GpuEngine

pytestmark = pytest.mark.gpu

TILE_SPANS, TRIP_TILES, CHUNK, TILE = mark_shape()
G = 8                                                               # guard entries on either side of every output
NAMES = ("out", "out_off", "span_new", "doc_run_off")
DTYPES = {"out": torch.uint8, "out_off": torch.int64, "span_new": torch.int32, "doc_run_off": torch.int64}


@pytest.fixture(scope="module")
def eng():
    e = Engine()
    yield e
    e.close()


_REF = {}


def reference(case):
    if case.name not in _REF:
        _REF[case.name] = M.expected(case)
    return _REF[case.name]


def marker_byte(case):
    return (case.open + case.close + b"<")[0]


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

    def call(self, e, outs=None, cap_bytes=0, flags=0, handle=None, open=-1, close=-1, open_len=None, close_len=None):
        """the raw call -> (rc, n_runs, total); outs: name -> tensor"""
        outs = outs or {}
        m, total = C.c_uint64(0), C.c_uint64(0)
        p = {k: (outs[k].data_ptr() if outs.get(k) is not None else None) for k in NAMES}
        o = self.case.open if open == -1 else open
        c = self.case.close if close == -1 else close
        torch.cuda.synchronize()
        rc = _lib.load().gft_mark_spans_device(
            handle or e._h, self.text.data_ptr(), self.d_off.data_ptr(), self.n, self.d_so.data_ptr(),
            self.d_st.data_ptr() if self.st.size else None, self.d_ln.data_ptr() if self.ln.size else None,
            o or None, len(o or b"") if open_len is None else open_len, c or None, len(c or b"") if close_len is None else close_len, flags,
            p["out"], cap_bytes, p["out_off"], p["span_new"], p["doc_run_off"], C.byref(m), C.byref(total))
        return rc, int(m.value), int(total.value)

    def sizes(self, total):
        return {"out": total, "out_off": self.n + 1, "span_new": self.st.size, "doc_run_off": self.n + 1}

    def guarded(self, sizes, shift=0):
        """name -> (allocation filled with the pattern, the view the call gets): G entries of guard on either side; the byte output
        `shift` bytes further into the 16-byte grid"""
        full, view = {}, {}
        pat = self.fill if self.fill else 0x5A
        for k, n in sizes.items():
            extra = G + shift if k == "out" else 0                  # (the byte output begins `shift` behind a 16-byte border)
            t = torch.empty(n + 2 * G + extra, dtype=DTYPES[k], device="cuda")
            assert t.data_ptr() % 16 == 0
            t.view(torch.uint8).fill_(pat)
            full[k], view[k] = t, t[G + extra:G + extra + n]
        return full, view, pat

    def run(self, e, cap_bytes=None, omit=(), shift=0):
        """count, then fill guarded tensors -> a dict like the reference's, the text cut to what the cap allows; the guards checked"""
        rc, m, total = self.call(e)
        assert rc == 0, _lib.load().gft_last_error(e._h)
        cb = total if cap_bytes is None else cap_bytes
        sizes = self.sizes(min(total, cb))
        full, view, pat = self.guarded(sizes, shift)
        for k in omit:
            view[k] = None
        rc, m2, total2 = self.call(e, view, cb if "out" not in omit else 0)
        assert rc == 0 and (m2, total2) == (m, total), _lib.load().gft_last_error(e._h)
        got = {"n_runs": m, "total": total}
        for k in NAMES:
            raw = full[k].view(torch.uint8).cpu().numpy()
            item = full[k].element_size()
            extra = G + shift if k == "out" else 0
            lo, hi = (G + extra) * item, (G + extra + sizes[k]) * item
            assert (raw[:lo] == pat).all() and (raw[hi:] == pat).all(), "%s: a store outside the output" % k
            if k in omit:
                assert (raw == pat).all(), "%s: not passed, yet written" % k
            got[k] = None if k in omit else view[k].cpu().numpy().tolist()
        if got["out"] is not None:
            got["out"] = bytes(got["out"])
        return got


def assert_same(got, want, what):
    for k in ("n_runs", "total", "out") + M.ARRAYS:
        if got[k] != want[k]:
            if k == "out":
                i = next((j for j, (a, b) in enumerate(zip(got[k], want[k])) if a != b), min(len(got[k]), len(want[k])))
                raise AssertionError("%s: out differs at byte %d: %r, expected %r" % (what, i, got[k][max(i - 8, 0):i + 24], want[k][max(i - 8, 0):i + 24]))
            raise AssertionError("%s: %s differs" % (what, k))


def test_the_reference_is_not_vacuous_and_the_shape_is_the_headers():
    assert M.assert_not_vacuous()
    assert (CHUNK, TILE) == (M.CHUNK, M.TILE) and M.TRIP == 64 * CHUNK and M.MARK_MAX == 255


FIXED = M.fixed_cases()
RESIDUES = (0, 1, 3, 8, 15)
SHIFTS = (0, 1, 7, 15)


@pytest.mark.parametrize("i", range(len(FIXED)), ids=[c.name for c in FIXED])
def test_fixed_case(eng, i):
    case = FIXED[i]
    want = reference(case)
    for fill in (0x00, marker_byte(case)):
        # the placement cases say where the insertions fall in the OUTPUT's grid: the output stays on it; the text moves
        at = RESIDUES[(i + (fill != 0)) % len(RESIDUES)]
        assert_same(OnDevice(case, fill, at).run(eng), want, "%s, fill %#x, text at +%d" % (case.name, fill, at))


@pytest.mark.parametrize("shift", SHIFTS[1:])
def test_output_shifted(eng, shift):
    for name in ("straddle_tile", "one_byte_runs", "markers_len_17", "text_residue_5", "many_insertions_in_tile"):
        case = next(c for c in FIXED if c.name == name)
        for fill in (0x00, marker_byte(case)):
            assert_same(OnDevice(case, fill, shift % 3).run(eng, shift=shift), reference(case), "%s, out at +%d" % (name, shift))


@pytest.mark.parametrize("at", RESIDUES)
def test_text_placement(eng, at):
    """the text at every residue, behind lead bytes (doc_off[0] != 0)"""
    for name in ("straddle_trip", "touch_across_docs", "text_residue_8"):
        case = next(c for c in FIXED if c.name == name)
        case = case.but(case.name + ", lead", lead=case.lead + 5)
        want = M.expected(case)
        for fill in (0x00, marker_byte(case)):
            assert_same(OnDevice(case, fill, at).run(eng, shift=(at * 5) % 16), want, "%s, fill %#x, at +%d" % (name, fill, at))


def test_random_batches(eng):
    for case in M.random_cases(5, 30):
        assert_same(OnDevice(case, marker_byte(case), case.lead % 3).run(eng, shift=case.lead % 16), M.expected(case), case.name)


COUNTS = M.count_cases(TILE_SPANS, TRIP_TILES)


@pytest.mark.parametrize("i", range(len(COUNTS)), ids=[c.name for c in COUNTS])
def test_span_counts_round_the_walks_borders(eng, i):
    case = COUNTS[i]
    got = OnDevice(case, marker_byte(case), 3).run(eng, shift=9)
    assert_same(got, reference(case), case.name)
    assert got["n_runs"] > len(case.spans[0]) // 2


def test_cap_protocol(eng):
    case = next(c for c in FIXED if c.name == "straddle_tile")
    want = reference(case)
    m, total = want["n_runs"], want["total"]
    d = OnDevice(case, marker_byte(case), 3)
    assert d.call(eng) == (0, m, total)                              # count only
    assert_same(d.run(eng, total), want, "an exact cap")
    o = TILE - 2                                                     # where the first open begins in the output
    assert want["out"][o:o + 4] == b"<em>" and want["out"][o + 12:o + 17] == b"</em>"
    for cb in (1, 100, o + 2, o + 14, 96, 107, TILE, o + 4, total - 1):   # inside text, inside open, inside close, at a chunk border (+0, +5)
        for shift in (0, 5):
            got = d.run(eng, cap_bytes=cb, shift=shift)               # (run checks the guards behind the cap)
            assert got["out"] == want["out"][:cb], cb
            assert all(got[k] == want[k] for k in M.ARRAYS), cb


@pytest.mark.parametrize("name", NAMES)
def test_every_output_null_on_its_own(eng, name):
    case = next(c for c in FIXED if c.name == "touch_across_docs")
    want = reference(case)
    got = OnDevice(case).run(eng, omit=(name,))
    for k in NAMES:
        if k != name:
            assert got[k] == want[k], k


def test_refusals_write_nothing_and_leave_the_handle_usable(eng):
    L = _lib.load()
    base = COUNTS[2]                                                # one span above a tile: the bad pair lies in the last tile
    good = reference(base)
    spans1 = list(base.spans[1])
    order = spans1[:-2] + [spans1[-1], spans1[-2]]                  # ends that descend
    past = spans1[:-1] + [(spans1[-1][0], len(base.docs[1]))]       # a span past its document's end
    sizes = OnDevice(base).sizes(good["total"])

    def refused(d, what, code=_lib.GFT_E_INVALID, **kw):
        full, view, pat = d.guarded(sizes)
        rc, m, total = d.call(eng, view, good["total"], **kw)
        assert rc == code and (m, total) == (0, 0), what
        for k in NAMES:
            assert (full[k].view(torch.uint8).cpu().numpy() == pat).all(), "%s: %s was written" % (what, k)
        assert_same(OnDevice(base).run(eng), good, "after the refusal of " + what)

    for name, sp in (("order", order), ("past the end", past)):
        refused(OnDevice(base.but(name, spans=[base.spans[0], sp]), 0x3C), name)
    d = OnDevice(base)
    refused(d, "flags", flags=1)
    refused(d, "flags, high bit", flags=0x80000000)
    refused(d, "a long open", open=b"x" * 256)
    refused(d, "a long close", close=b"x" * 300)
    refused(d, "a NULL open with a length", open=None, open_len=3)
    refused(d, "a NULL close with a length", close=None, close_len=1)
    multi = Engine(devices=[0, 0])
    try:
        refused(d, "a handle over several devices", code=_lib.GFT_E_UNSUPPORTED, handle=multi._h)
    finally:
        multi.close()
    assert d.call(eng, {}, 5)[0] == _lib.GFT_E_INVALID              # cap_bytes without an output
    # outputs that are inputs, outputs that overlap each other
    assert d.call(eng, {"span_new": d.d_st})[0] == _lib.GFT_E_INVALID
    assert d.call(eng, {"out": d.text[4:]}, 8)[0] == _lib.GFT_E_INVALID
    assert d.call(eng, {"out_off": d.d_off})[0] == _lib.GFT_E_INVALID
    both = torch.zeros(8, dtype=torch.int64, device="cuda")
    assert d.call(eng, {"out_off": both, "doc_run_off": both[1:]})[0] == _lib.GFT_E_INVALID
    # offsets that descend
    d2 = OnDevice(M.Case("two", [b"abcdef", b"ghij"], [[(1, 1)], [(1, 1)]]))
    d2.d_off = torch.tensor([0, 12, 10], dtype=torch.int64, device="cuda")
    assert d2.call(eng)[0] == _lib.GFT_E_INVALID
    d2 = OnDevice(M.Case("three", [b"abcdef", b"ghij", b"k"], [[(1, 1)], [(1, 1)], []]))
    d2.d_so = torch.tensor([0, 2, 1, 2], dtype=torch.int64, device="cuda")
    assert d2.call(eng)[0] == _lib.GFT_E_INVALID and b"span offsets descend" in L.gft_last_error(eng._h)
    # a document that would reach 4 GiB once marked: found from the offsets alone, no text is read
    d2 = OnDevice(M.Case("big", [b"abc"], [[(1, 1)]]))
    d2.d_off = torch.tensor([0, (1 << 32) - 8], dtype=torch.int64, device="cuda")
    assert d2.call(eng)[0] == _lib.GFT_E_INVALID and b"4 GiB once marked" in L.gft_last_error(eng._h)
    # no documents: the offsets are not read; the two offset arrays get their 0
    oo = torch.full((2,), 7, dtype=torch.int64, device="cuda")
    ro = torch.full((2,), 7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert L.gft_mark_spans_device(eng._h, None, None, 0, None, None, None, b"<", 1, b">", 1, 0, None, 0, oo.data_ptr(), None, ro.data_ptr(),
                                   None, None) == 0
    assert oo.cpu().tolist() == [0, 7] and ro.cpu().tolist() == [0, 7]
    assert_same(OnDevice(base).run(eng), good, "after every refusal")


def test_profile_names_and_last_nonascii(eng):
    L = _lib.load()
    case = next(c for c in FIXED if c.name == "straddle_tile")
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
    assert_same(d.run(eng), reference(case), case.name)
    for name in ("mark_runs", "mark_scan", "mark_place"):
        assert eng.profile_read(name)[1] == 2, name                 # (run calls twice: count, fill)
    assert eng.profile_read("mark_copy")[1] == 1 and eng.profile_read("select_copy")[1] == 0 and eng.profile_read("excerpt_copy")[1] == 0
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


def as_case(name, docs, so, st, ln, open=b"<em>", close=b"</em>"):
    so, st, ln = (t.cpu().numpy().astype(np.int64) for t in (so, st, ln))
    so = so - so[0]
    return M.Case(name, docs, [list(zip(st[so[d]:so[d + 1]].tolist(), ln[so[d]:so[d + 1]].tolist())) for d in range(len(docs))], open, close)


def tensors_as_result(t):
    out, out_off, span_new, doc_run_off = t[:4]
    return {"n_runs": int(doc_run_off[-1]), "total": int(out.numel()), "out": out.cpu().numpy().tobytes(), "out_off": out_off.cpu().tolist(),
            "span_new": span_new.cpu().tolist(), "doc_run_off": doc_run_off.cpu().tolist()}


def splice(line, spans, open, close):
    """a line with markers round the (start, end, keyword) hits, by the reference"""
    return M.expected(M.Case("line", [line], [[(a, b - a) for a, b, _ in spans]], open, close))["out"]


def test_chain_split_process_spans_mark_redact_and_twice(finder):
    lines = [ln + b"\n" for ln in LOG]
    data = b"".join(lines)
    buf = resident(data)
    off, bm = finder.ProcessLinesDevice(buf, len(data))
    so, st, ln, tm, low = finder.SpansDevice(buf, off, bm)
    assert not low and int(st.numel()) > 20
    t = finder.MarkDevice(buf, off, so, st, ln, low, False, b"**", b"**")
    case = as_case("log", lines, so, st, ln, b"**", b"**")
    want = M.expected(case)
    assert_same(tensors_as_result(t), want, "split -> process -> spans -> mark")
    assert t[4] is False and want["n_runs"] > 10
    # ... against the Python splice of SpansLines(source=True)
    idx, spans, _ = finder.SpansLines(data, source=True)
    by_line = dict(zip(idx.tolist(), spans))
    assert want["out"] == b"".join(splice(line, by_line.get(d, []), b"**", b"**") for d, line in enumerate(lines))
    # ... and (out, out_off, span_off, span_new, span_len) is what the redaction takes: exactly the hit bytes, every marker intact
    out, out_off, span_new = t[:3]
    masked = out.clone()
    L = _lib.load()
    torch.cuda.synchronize()
    assert L.gft_redact_spans_device(finder.engine_handle(), masked.data_ptr(), out_off.data_ptr(), len(lines), so.data_ptr(), span_new.data_ptr(),
                                     ln.data_ptr(), ord("#")) == 0
    hidden = M.Case("hidden", [bytes(b"#"[0] if any(a <= i < a + n for a, n in sp) else c for i, c in enumerate(doc))
                               for doc, sp in zip(case.docs, case.spans)], case.spans, b"**", b"**")
    assert masked.cpu().numpy().tobytes() == M.expected(hidden)["out"] != want["out"]
    # ... and of this call itself: marks round the marked hits, which nests
    t2 = finder.MarkDevice(out, out_off, so, span_new, ln, False, False, b"[", b"]")
    docs2 = [want["out"][a:b] for a, b in zip(want["out_off"], want["out_off"][1:])]
    assert_same(tensors_as_result(t2), M.expected(as_case("twice", docs2, so, span_new, ln, b"[", b"]")), "mark -> mark")
    assert b"**[" in t2[0].cpu().numpy().tobytes()


def test_chain_select_and_route_with_row_idx(finder):
    lines = [ln + b"\n" for ln in LOG]
    data = b"".join(lines)
    want_mask = finder.want_mask([0, 1])
    out, out_off, doc_idx, off, bm = finder.SelectLinesDevice(resident(data), len(data), want_mask)
    so, st, ln, tm, low = finder.SpansDevice(out, out_off, bm, want_mask, row_idx=doc_idx)
    picked = [lines[i] for i in doc_idx.cpu().tolist()]
    t = finder.MarkDevice(out, out_off, so, st, ln, low, False)
    assert_same(tensors_as_result(t), M.expected(as_case("selected", picked, so, st, ln)), "process -> select -> spans -> mark")
    assert len(picked) >= 9 and int(t[3][-1]) >= len(picked)
    # a route's bucket run as the batch: doc_off[0] != 0
    out, out_off, doc_idx, bucket_doc, bucket_byte, off, bm = finder.RouteLinesDevice(resident(data), len(data), [[0], [1]])
    b0, b1 = int(bucket_doc[1]), int(bucket_doc[2])
    assert b1 > b0 > 0 and int(bucket_byte[1]) > 0
    run_off, run_idx = out_off[b0:b1 + 1].contiguous(), doc_idx[b0:b1].contiguous()
    so, st, ln, tm, low = finder.SpansDevice(out, run_off, bm, finder.want_mask([1]), row_idx=run_idx)
    picked = [lines[i] for i in run_idx.cpu().tolist()]
    t = finder.MarkDevice(out, run_off, so, st, ln, low, False)
    assert_same(tensors_as_result(t), M.expected(as_case("bucket", picked, so, st, ln)), "a route's bucket run")


def test_chain_excerpt_mark(finder):
    lines = [ln + b"\n" for ln in LOG]
    data = b"".join(lines)
    buf = resident(data)
    off, bm = finder.ProcessLinesDevice(buf, len(data))
    so, st, ln, tm, low = finder.SpansDevice(buf, off, bm)
    out, exc_off, exc_doc, exc_start, exc_span_off, span_rel = finder.ExcerptsDevice(buf, off, so, st, ln, low, False, 6, 4)[:6]
    blob, eo = out.cpu().numpy().tobytes(), exc_off.cpu().tolist()
    t = finder.MarkDevice(out, exc_off, exc_span_off, span_rel, ln, False, False)
    case = as_case("excerpts", [blob[a:b] for a, b in zip(eo, eo[1:])], exc_span_off, span_rel, ln)
    assert_same(tensors_as_result(t), M.expected(case), "excerpt -> mark")
    assert len(case.docs) > 10


def test_highlight_lines_of_a_lowered_batch(finder):
    lines = [ln + b"\n" for ln in LOG]
    lines[2] = "GET /café 403 ÿ\n".encode()
    lines[3] = "KERNEL: OOM-killer invoked by CAFÉ\n".encode()
    lines[6] = "Ⱥ grows, then a password for root ⱥⱥⱥ\n".encode()     # U+023A grows: what follows moves to the right
    data = b"".join(lines)
    for source in (True, False):
        idx, spans, low = finder.SpansLines(data, source=source)
        got, glow = finder.HighlightLines(data, b"\x1b[1m", b"\x1b[0m", source=source)
        assert low and glow
        by_line = dict(zip(idx.tolist(), spans))
        if source:
            texts = lines
        else:
            texts = [ln.decode().lower().encode() for ln in lines]
            for d, sp in by_line.items():
                for a, b, kw in sp:
                    assert texts[d][a:b] == kw, (d, a, b, kw)      # (Python's lower() agrees with strings.ToLower on these lines)
        assert got == b"".join(splice(t, by_line.get(d, []), b"\x1b[1m", b"\x1b[0m") for d, t in enumerate(texts)), source
        assert got.count(b"\x1b[1m") > 10
    # an ASCII batch: both forms agree and nothing is lowered
    data = b"".join(ln + b"\n" for ln in LOG)
    a, b = finder.HighlightLines(data, source=True), finder.HighlightLines(data, source=False)
    assert a == b and a[1] is False and b"<em>password</em>" in a[0]


def test_excerpt_lines_with_marks(finder):
    lines = [ln + b"\n" for ln in LOG]
    lines[2] = "GET /café 403 ÿ\n".encode()
    data = b"".join(lines)
    idx, plain, low = finder.ExcerptLines(data, before=9, after=9)
    idx2, marked, low2 = finder.ExcerptLines(data, before=9, after=9, mark=(b"<b>", b"</b>"))
    assert idx.tolist() == idx2.tolist() and low == low2 and any(plain)
    for per_plain, per_marked in zip(plain, marked):
        assert len(per_plain) == len(per_marked)
        for (s0, text, hits), (s1, mtext, mhits) in zip(per_plain, per_marked):
            want = M.expected(M.Case("excerpt", [text], [[(a, b - a) for a, b, _ in hits]], b"<b>", b"</b>"))
            assert s0 == s1 and mtext == want["out"]
            assert [(a, b - a, kw) for a, b, kw in mhits] == [(n, b - a, kw) for n, (a, b, kw) in zip(want["span_new"], hits)]
            for (a, b, _), (c, d, _) in zip(hits, mhits):
                assert mtext[c:d] == text[a:b] and mtext[:c].endswith(b"<b>") == (mtext[c - 3:c] == b"<b>")
