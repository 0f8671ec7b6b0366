"""Spans of a lowered batch mapped back to the source text on the device (csrc/gft_lowermap.hip, the table form of k_lower):
gft_map_spans_to_source_device bit for bit against the host walk (itself held to the sequential reference by
tests/test_lowermap_host.py) on the ToLower batches, random documents, the piece / trip / unit borders and a text that begins 1, 3
and 7 bytes into its allocation; a refusal that leaves the arrays untouched; and the callers: Finder.SpansLines / RedactLines /
SpansDevice with source=True against the reference of lowermap_cases.py, and the cap protocol of
gft_finder_hit_spans_source_device into guarded tensors.  All comparisons are exact."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before libgft.so is loaded: one HIP runtime)

import lowermap_cases as M
import tolower_cases as TC
from gofindthem_amd import _lib
from gofindthem_amd.engine import Engine, GftError, map_spans_to_source_host
from gofindthem_amd.finder import EmptyRgxEngine, Finder, GpuEngine

pytestmark = pytest.mark.gpu

GUARD32 = -0x5A5A5A5B


@pytest.fixture(scope="module")
def eng():
    e = Engine()
    yield e
    e.close()


class OnDevice:
    """a batch and the lowered spans of it on the device, the text `at` bytes into an allocation filled with 0xC3 / 0x89"""

    def __init__(self, docs, spans, lead=0, at=0):
        self.blob, self.off = TC.pack(list(docs), lead)
        self.so, self.st, self.ln = M.flat(spans)
        buf = torch.full((at + self.blob.size + 16,), 0x89, dtype=torch.uint8, device="cuda")
        buf[:at] = 0xC3
        buf[at:at + self.blob.size] = torch.from_numpy(self.blob).cuda()
        self.text = buf[at:]
        self.d_off = torch.from_numpy(self.off.astype(np.int64)).cuda()
        self.d_so = torch.from_numpy(self.so.astype(np.int64)).cuda()
        self.d_st = torch.from_numpy(self.st.view(np.int32).copy()).cuda()
        self.d_ln = torch.from_numpy(self.ln.view(np.int32).copy()).cuda()

    def run(self, e):
        e.map_spans_to_source_device(self.text, self.d_off, self.d_so, self.d_st, self.d_ln)
        return self.got()

    def got(self):
        return self.d_st.cpu().numpy().view(np.uint32), self.d_ln.cpu().numpy().view(np.uint32)

    def host(self):
        st, ln = self.st.copy(), self.ln.copy()
        map_spans_to_source_host(self.blob, self.off, self.so, st, ln)
        return st, ln


def assert_device_is_host(e, docs, spans, what, lead=0, at=0):
    d = OnDevice(docs, spans, lead, at)
    got, want = d.run(e), d.host()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what
    return want


def test_device_equals_the_host_walk(eng):
    moved = 0
    for name, docs in TC.edge_batches().items():
        spans = [M.every_byte(doc, n_random=20, seed=i) for i, doc in enumerate(docs)]
        w = assert_device_is_host(eng, docs, spans, name, lead=5 if name == "cut_runes" else 0)
        moved += int((w[0] != M.flat(spans)[1]).sum())
    assert moved > 1000                                             # (the map is not the identity on these batches)
    docs = TC.random_docs(300)
    spans = [M.every_byte(doc, n_random=20, seed=i) for i, doc in enumerate(docs)]
    for at in (0, 1, 3, 7):
        assert_device_is_host(eng, docs, spans, "random, text at +%d" % at, lead=at, at=at)
    # ... and against the sequential reference itself, once
    d = OnDevice(docs, spans)
    got, ref = d.run(eng), M.expected(docs, spans)
    assert np.array_equal(got[0], ref[1]) and np.array_equal(got[1], ref[2])


def test_runes_at_the_piece_trip_and_unit_borders(eng):
    for border in ("piece", "trip"):
        placed = M.border_docs([border])
        assert_device_is_host(eng, [doc for doc, _ in placed], [M.around(doc, a) for doc, a in placed], border, at=3)
    # the documents of 8.3 KB, two work units each: every seventh rune of the list at the unit figure and at the cut between the
    # document's two units
    for border in ("unit", "unit cut"):
        placed = M.border_docs([border], every=7)
        assert len(placed) >= 15
        docs = [doc for doc, _ in placed]
        want = assert_device_is_host(eng, docs, [M.around(doc, a) for doc, a in placed], border, lead=1, at=1)
        ref = M.expected(docs, [M.around(doc, a) for doc, a in placed])
        assert np.array_equal(want[0], ref[1]) and np.array_equal(want[1], ref[2])


def test_degenerate_shapes_and_identity(eng):
    none = (np.zeros(0, np.int64), np.zeros(0, np.int64))
    docs = [b"", b"K", b"\xff", "İ".encode()]
    spans = [(np.zeros(1, np.int64), np.zeros(1, np.int64)), (np.array([0, 0, 1]), np.array([1, 0, 0])),
             (np.array([0, 1, 2, 3, 0]), np.array([0, 0, 0, 0, 3])), (np.array([0, 1, 0]), np.array([0, 0, 1]))]
    assert_device_is_host(eng, docs, spans, "tiny")
    assert_device_is_host(eng, docs, [none] * 4, "no spans")
    L = _lib.load()
    assert L.gft_map_spans_to_source_device(eng._h, None, None, 0, None, None, None) == 0
    doc = ("İstanbul Ⱥ KELVIN K ".encode() + b"\xff ") * 12 + "İK".encode() * 30
    s = np.arange(130) % M.lowered_len(doc)
    assert_device_is_host(eng, [b"x", doc, b""], [none, (s, np.ones(130, np.int64)), none], "130 spans")
    docs = [("É%d İ" % i).encode() for i in range(130)]
    assert_device_is_host(eng, docs, [(np.array([i % 3]), np.array([2])) for i in range(130)], "130 documents")
    # fold-safe text: the spans come back as they went in
    docs = M.fold_safe_docs()
    spans = []
    for doc in docs:
        cuts = np.concatenate([M.runes(doc).a, [len(doc)]])
        spans.append((cuts[:-1][:50], np.diff(cuts)[:50]))
    d = OnDevice(docs, spans)
    eng.profile(True)
    eng.profile_reset()
    got = d.run(eng)
    assert np.array_equal(got[0], d.st) and np.array_equal(got[1], d.ln) and d.st.size > 100
    # the two stages of the call, by name: count pass, prefix sum and table pass under one, check and write pass under the other
    assert eng.profile_read("lowermap_table")[1] == 3 and eng.profile_read("lowermap_spans")[1] == 1
    assert eng.profile_read("lower_count")[1] == 0 and eng.profile_read("lower_write")[1] == 0
    eng.profile(False)


def test_a_refusal_on_the_device_writes_nothing(eng):
    docs = ["CAFÉ İ one".encode(), "İİ two Ⱥ".encode(), b"three \xff" + b"." * 200]
    for bad in (1, 2):
        spans = [(np.array([0, 2]), np.array([3, 1]))] * 3
        B = M.lowered_len(docs[bad])
        spans[bad] = (np.array([0, B - 1, 1]), np.array([1, 2, 1]))  # one byte past the lowered end: far inside every allocation
        d = OnDevice(docs, spans)
        with pytest.raises(GftError) as ei:
            d.run(eng)
        assert ei.value.code == _lib.GFT_E_INVALID
        got = d.got()
        assert np.array_equal(got[0], d.st) and np.array_equal(got[1], d.ln)
    # overlapping span arrays are refused before any launch; the handle works afterwards
    d = OnDevice(docs, [(np.array([0, 2]), np.array([3, 1]))] * 3)
    L = _lib.load()
    rc = L.gft_map_spans_to_source_device(eng._h, d.text.data_ptr(), d.d_off.data_ptr(), 3, d.d_so.data_ptr(), d.d_st.data_ptr(), d.d_st.data_ptr() + 8)
    assert rc == _lib.GFT_E_INVALID
    got = d.got()
    assert np.array_equal(got[0], d.st) and np.array_equal(got[1], d.ln)
    want = d.host()
    got = d.run(eng)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---- the finder ------------------------------------------------------------------------------------------------------------------
LOG = [b"GET /index.html 200", b"POST /login 401 bad password for root", b"GET /admin 403", b"kernel: oom-killer invoked", b"",
       b"POST /login 200 root", b"GET /health 200", b"sshd: Failed password for root from 10.0.0.7", b"cron: job done"] * 3
LOG_EXPRS = ['"password" and "root"', '"403" or "oom"', '"GET" and not "200"', 'inord("POST" and "login")', '"café" or "ÿ"']


def log_lines(kind):
    lines = [ln + b"\n" for ln in LOG]
    if kind != "ascii":
        lines[2] = "GET /café 403 ÿ\n".encode()
    if kind == "lowered":
        lines[3] = "KERNEL: OOM-killer İnvoked by CAFÉ\n".encode()     # U+0130 shrinks: what follows moves to the left
        lines[6] = "Ⱥ grows, then a password for root\n".encode()                # U+023A grows: what follows moves to the right
        lines[7] = b"\x80 oom behind a lone continuation byte 403\n"             # one byte becomes three
    return lines


def mapped_reference(lines, idx, spans):
    """SpansLines' lowered (start, end, keyword) lists through the reference map"""
    out = []
    for d, sp in zip(idx.tolist(), spans):
        s = np.array([a for a, _, _ in sp], np.int64)
        n = np.array([b - a for a, b, _ in sp], np.int64)
        ms, mn = M.map_spans(lines[d], s, n)
        out.append([(int(a), int(a + k), kw) for a, k, (_, _, kw) in zip(ms, mn, sp)])
    return out


@pytest.fixture(scope="module")
def finder():
    f = Finder(GpuEngine.__new__(GpuEngine), EmptyRgxEngine(), False)
    f.AddExpressions(LOG_EXPRS)
    yield f
    f.close()


def test_finder_source_spans_and_redaction_of_a_lowered_batch(finder):
    lines = log_lines("lowered")
    data = b"".join(lines)
    idx, spans, low = finder.SpansLines(data)
    sidx, sspans, slow = finder.SpansLines(data, source=True)
    assert low and slow and sidx.tolist() == idx.tolist() and any(spans)
    ref = mapped_reference(lines, idx, spans)
    assert sspans == ref
    assert any(a[0] != b[0] for x, y in zip(spans, sspans) for a, b in zip(x, y))          # some start moved
    assert {3, 6, 7} <= set(idx.tolist())
    # every source span shows the keyword, lower-cased, in the caller's line
    for d, sp in zip(sidx.tolist(), sspans):
        for a, b, kw in sp:
            assert TC.ref_lower(lines[d][a:b]) == kw, (d, a, b, kw)
    masked, mlow = finder.RedactLines(data, source=True)
    assert mlow and len(masked) == len(data)
    inside = np.zeros(len(data), bool)
    o = 0
    line_at = {}
    for d, ln in enumerate(lines):
        line_at[d] = o
        o += len(ln)
    for d, sp in zip(idx.tolist(), ref):
        for a, b, _ in sp:
            inside[line_at[d] + a:line_at[d] + b] = True
    got, src = np.frombuffer(masked, np.uint8), np.frombuffer(data, np.uint8)
    assert inside.any() and (got[inside] == ord("*")).all() and np.array_equal(got[~inside], src[~inside])
    assert "KERNEL: ***-killer İnvoked by *****\n".encode() in masked      # (the letters outside the spans keep their case)
    assert masked != finder.RedactLines(data)[0]
    # another mask byte, one column
    w = finder.want_mask([1])
    m2, _ = finder.RedactLines(data, w, b"#", source=True)
    assert len(m2) == len(data) and b"#" in m2 and b"password" in m2


@pytest.mark.parametrize("kind", ["ascii", "fold-safe"])
def test_finder_source_changes_nothing_on_a_fold_safe_batch(finder, kind):
    data = b"".join(log_lines(kind))
    a, b = finder.SpansLines(data), finder.SpansLines(data, source=True)
    assert a[0].tolist() == b[0].tolist() and a[1] == b[1] and any(a[1]) and a[2] is False and b[2] is False
    assert finder.RedactLines(data) == finder.RedactLines(data, source=True)


def resident(data):
    buf = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda")
    buf[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    return buf


def test_source_spans_compose_with_a_select(finder):
    lines = log_lines("lowered")
    data = b"".join(lines)
    want = finder.want_mask([0, 1])
    out, out_off, doc_idx, off, bm = finder.SelectLinesDevice(resident(data), len(data), want)
    so, st, ln, tm, low = finder.SpansDevice(out, out_off, bm, want, row_idx=doc_idx, source=True)
    lo_so, lo_st, lo_ln, lo_tm, low2 = finder.SpansDevice(out, out_off, bm, want, row_idx=doc_idx)
    assert low and low2 and so.cpu().tolist() == lo_so.cpu().tolist() and tm.cpu().tolist() == lo_tm.cpu().tolist()
    picked = [lines[i] for i in doc_idx.cpu().tolist()]
    assert {3, 6, 7} <= set(doc_idx.cpu().tolist())
    offs = so.cpu().numpy()
    a, n = lo_st.cpu().numpy().astype(np.int64), lo_ln.cpu().numpy().astype(np.int64)
    ref = M.expected(picked, [(a[offs[d]:offs[d + 1]], n[offs[d]:offs[d + 1]]) for d in range(len(picked))])
    assert np.array_equal(st.cpu().numpy().view(np.uint32), ref[1]) and np.array_equal(ln.cpu().numpy().view(np.uint32), ref[2])
    assert (ref[1] != a).any()


def test_cap_protocol_of_the_source_call(finder):
    lines = log_lines("lowered")
    data = b"".join(lines)
    buf = resident(data)
    off, bm = finder.ProcessLinesDevice(buf, len(data))
    n = int(off.numel()) - 1
    so, st, ln, tm, low = finder.SpansDevice(buf, off, bm, source=True)
    total = int(st.numel())
    assert low and total > 12
    L = _lib.load()
    for cap in (total - 1, 5, 1):
        d_so = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
        arrs = [torch.full((total + 8,), GUARD32, dtype=torch.int32, device="cuda") for _ in range(3)]
        got_total, lowered = C.c_uint64(0), C.c_int(0)
        torch.cuda.synchronize()
        rc = L.gft_finder_hit_spans_source_device(finder._h, buf.data_ptr(), off.data_ptr(), n, bm.data_ptr(), None, None, d_so.data_ptr(),
                                                  arrs[0].data_ptr(), arrs[1].data_ptr(), arrs[2].data_ptr(), cap, C.byref(got_total), C.byref(lowered))
        assert rc == 0 and got_total.value == total and lowered.value == 1
        assert d_so.cpu().tolist() == so.cpu().tolist()
        for got, full in zip(arrs, (st, ln, tm)):
            g = got.cpu().numpy()
            assert np.array_equal(g[:cap], full.cpu().numpy()[:cap]) and (g[cap:] == GUARD32).all(), cap
    # spans are to be written but the map has no offsets to go by
    arrs = [torch.full((total,), GUARD32, dtype=torch.int32, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    rc = L.gft_finder_hit_spans_source_device(finder._h, buf.data_ptr(), off.data_ptr(), n, bm.data_ptr(), None, None, None, arrs[0].data_ptr(),
                                              arrs[1].data_ptr(), arrs[2].data_ptr(), total, None, None)
    assert rc == _lib.GFT_E_INVALID and (arrs[0].cpu().numpy() == GUARD32).all()
