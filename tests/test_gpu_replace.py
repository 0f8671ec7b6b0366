"""Replace on the device: gft_replace_spans_device against the reference of replace.py, bit for bit, on every fixed case -- with
0x00 and with a byte of a replacement round the text and round every output, in guarded tensors, the output at several residues
of the 16-byte grid --, the span counts round the walk's borders and random batches; both caps; every output NULL on its own; the
refusals, which must leave every output untouched and the handle usable, a bad key found on the device among them; the chains
spans -> replace (against a splice of SpansLines in Python), select and route with row_idx -> spans -> replace, replace ->
redact / mark / excerpt on the handed-back run list and replace twice; Finder.ReplaceLines with bytes, with a dict, over a batch
that is lowered and with whole_words; the profile names and gft_last_nonascii.  All comparisons are exact."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before libgft.so is loaded: one HIP runtime)

import replace as R
from gofindthem_amd import _lib
from gofindthem_amd.engine import Engine, replace_shape, replace_table
from gofindthem_amd.finder import EmptyRgxEngine, Finder, GpuEngine

pytestmark = pytest.mark.gpu

TILE_SPANS, TRIP_TILES, CHUNK, TILE, WINDOW, LDS_TABLE = replace_shape()
G = 8                                                               # guard entries on either side of every output
NAMES = ("out", "out_off", "doc_run_off", "run_new", "run_len", "run_rep")
PER_RUN = NAMES[3:]
DTYPES = {"out": torch.uint8, "out_off": torch.int64, "doc_run_off": torch.int64, "run_new": torch.int32, "run_len": torch.int32,
          "run_rep": torch.int32}


@pytest.fixture(scope="module")
def eng():
    e = Engine()
    yield e
    e.close()


_REF = {}


def reference(case):
    if case.name not in _REF:
        _REF[case.name] = R.expected(case)
    return _REF[case.name]


def rep_byte(case):
    return (b"".join(case.reps) + b"<")[0]


class OnDevice:
    """a case on the device: the text `at` bytes into an allocation whose every other byte -- in front, the lead, the 64 bytes of
    slack -- holds `fill`; the span arrays behind span_lead entries and in front of span_tail entries no call may read"""

    def __init__(self, case, fill=0x00, at=0, span_lead=0, span_tail=0):
        self.case = case
        self.blob, self.off, self.so, self.st, self.ln, self.ky = case.arrays(fill, span_lead, span_tail)
        buf = torch.full((at + self.blob.size + 64,), fill, dtype=torch.uint8, device="cuda")
        if self.blob.size:
            buf[at:at + self.blob.size] = torch.from_numpy(self.blob.copy()).cuda()
        self.text = buf[at:]
        self.n = len(case.docs)
        self.d_off = torch.from_numpy(self.off.astype(np.int64)).cuda()
        self.d_so = torch.from_numpy(self.so.astype(np.int64)).cuda()
        self.d_st = torch.from_numpy(self.st.view(np.int32).copy()).cuda()
        self.d_ln = torch.from_numpy(self.ln.view(np.int32).copy()).cuda()
        self.d_ky = torch.from_numpy(self.ky.view(np.int32).copy()).cuda() if self.ky is not None else None
        self.rep_bytes, self.rep_off = replace_table(case.reps)
        self.key_rep = np.array(case.key_rep, dtype=np.uint32) if case.keyed and case.key_rep is not None else None
        self.fill = fill

    def call(self, e, outs=None, cap_bytes=0, cap_runs=0, flags=0, handle=None, **kw):
        """the raw call -> (rc, n_runs, total); outs: name -> tensor"""
        outs = outs or {}
        m, total = C.c_uint64(0), C.c_uint64(0)
        p = {k: (outs[k].data_ptr() if outs.get(k) is not None and outs[k].numel() else None) for k in NAMES}
        kr = kw.get("key_rep", self.key_rep)
        rep_off = kw.get("rep_off", self.rep_off)
        torch.cuda.synchronize()
        rc = _lib.load().gft_replace_spans_device(
            handle or e._h, self.text.data_ptr(), self.d_off.data_ptr(), self.n, self.d_so.data_ptr(),
            self.d_st.data_ptr() if self.st.size else None, self.d_ln.data_ptr() if self.ln.size else None,
            self.d_ky.data_ptr() if self.d_ky is not None and self.d_ky.numel() else None, kr.ctypes.data if kr is not None else None,
            kr.size if kr is not None else 0, kw.get("rep_bytes", self.rep_bytes) or None, rep_off.ctypes.data, kw.get("n_reps", rep_off.size - 1),
            flags, p["out"], cap_bytes, p["out_off"], p["doc_run_off"], p["run_new"], p["run_len"], p["run_rep"], cap_runs, C.byref(m),
            C.byref(total))
        return rc, int(m.value), int(total.value)

    def sizes(self, total, runs):
        return {"out": total, "out_off": self.n + 1, "doc_run_off": self.n + 1, "run_new": runs, "run_len": runs, "run_rep": runs}

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

    def run(self, e, cap_bytes=None, cap_runs=None, omit=(), shift=0):
        """count, then fill guarded tensors -> a dict like the reference's, cut to what the caps allow; the guards checked"""
        rc, m, total = self.call(e)
        assert rc == 0, _lib.load().gft_last_error(e._h)
        cb = total if cap_bytes is None else cap_bytes
        cr = m if cap_runs is None else cap_runs
        sizes = self.sizes(min(total, cb), min(m, cr))
        full, view, pat = self.guarded(sizes, shift)
        for k in omit:
            view[k] = None
        rc, m2, total2 = self.call(e, view, cb if "out" not in omit else 0, cr)
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
    for k in ("n_runs", "total", "out") + R.ARRAYS:
        if got[k] != want[k]:
            if k == "out":
                i = next((j for j, (a, b) in enumerate(zip(got[k], want[k])) if a != b), min(len(got[k]), len(want[k])))
                raise AssertionError("%s: out differs at byte %d: %r, expected %r" % (what, i, got[k][max(i - 8, 0):i + 24], want[k][max(i - 8, 0):i + 24]))
            raise AssertionError("%s: %s differs" % (what, k))


def test_the_reference_is_not_vacuous_and_the_shape_is_the_headers():
    assert R.assert_not_vacuous()
    assert (CHUNK, TILE) == (R.CHUNK, R.TILE) and R.TRIP == 64 * CHUNK and R.REPLACE_MAX == 255 and WINDOW == 64


FIXED = R.fixed_cases()
RESIDUES = (0, 1, 3, 8, 15)
SHIFTS = (0, 1, 7, 15)


def case_named(name):
    return next(c for c in FIXED if c.name == name)


@pytest.mark.parametrize("i", range(len(FIXED)), ids=[c.name for c in FIXED])
def test_fixed_case(eng, i):
    case = FIXED[i]
    want = reference(case)
    for fill in (0x00, rep_byte(case)):
        # the placement cases say where the runs fall in the OUTPUT's grid: the output stays on it; the text moves
        at = RESIDUES[(i + (fill != 0)) % len(RESIDUES)]
        assert_same(OnDevice(case, fill, at).run(eng), want, "%s, fill %#x, text at +%d" % (case.name, fill, at))


@pytest.mark.parametrize("shift", SHIFTS[1:])
def test_output_shifted(eng, shift):
    for name in ("straddle_tile", "sixteen_deleted", "sixteen_17_bytes", "rep_len_17", "text_residue_5", "many_runs_in_tile", "deleted_run_over_tile",
                 "touch_across_docs_deleted"):
        case = case_named(name)
        for fill in (0x00, rep_byte(case)):
            assert_same(OnDevice(case, fill, shift % 3).run(eng, shift=shift), reference(case), "%s, out at +%d" % (name, shift))


@pytest.mark.parametrize("at", RESIDUES)
def test_text_placement_behind_a_span_base(eng, at):
    """the text at every residue, behind lead bytes (doc_off[0] != 0), the spans behind a base (span_off[0] != 0)"""
    for name in ("straddle_trip", "touch_across_docs", "text_residue_8", "key_rep_given", "smallest_is_neither", "no_keys"):
        case = case_named(name)
        case = case.but(case.name + ", lead", lead=case.lead + 5)
        want = R.expected(case)
        for fill in (0x00, rep_byte(case)):
            assert_same(OnDevice(case, fill, at, 3, 2).run(eng, shift=(at * 5) % 16), want, "%s, fill %#x, at +%d" % (name, fill, at))


def test_random_batches(eng):
    for case in R.random_cases(5, 30):
        assert_same(OnDevice(case, rep_byte(case), case.lead % 3, case.lead % 4, 1).run(eng, shift=case.lead % 16), R.expected(case), case.name)


COUNTS = R.count_cases(TILE_SPANS, TRIP_TILES)


@pytest.mark.parametrize("i", range(len(COUNTS)), ids=[c.name for c in COUNTS])
def test_span_counts_round_the_walks_borders(eng, i):
    case = COUNTS[i]
    got = OnDevice(case, rep_byte(case), 3).run(eng, shift=9)
    assert_same(got, reference(case), case.name)
    assert got["n_runs"] > len(case.spans[0]) // 2


def test_cap_protocol(eng):
    case = case_named("straddle_tile")
    want = reference(case)
    m, total = want["n_runs"], want["total"]
    d = OnDevice(case, rep_byte(case), 3)
    assert d.call(eng) == (0, m, total)                              # count only
    assert_same(d.run(eng, total, m), want, "exact caps")
    o = TILE - 2                                                     # where the first replacement begins in the output
    assert want["out"][o:o + 6] == b"[NAME]" and m == 2
    for cb in (1, 100, o, o + 2, o + 5, o + 6, TILE, total - 1, total + 7):   # inside text, inside a replacement, at its ends, at a tile border
        for cr in (0, 1, 2, 5):
            got = d.run(eng, cap_bytes=cb, cap_runs=cr, shift=5 * (cr % 2))   # (run checks the guards behind the caps)
            assert got["out"] == want["out"][:cb], (cb, cr)
            assert got["out_off"] == want["out_off"] and got["doc_run_off"] == want["doc_run_off"]
            assert all(got[k] == want[k][:cr] for k in PER_RUN), (cb, cr)


@pytest.mark.parametrize("name", NAMES)
def test_every_output_null_on_its_own(eng, name):
    case = case_named("touch_across_docs")
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
    past = spans1[:-1] + [(spans1[-1][0], len(base.docs[1]), 0)]    # a span past its document's end
    bad_key = spans1[:-1] + [(spans1[-1][0], spans1[-1][1], 3)]     # an id at or past n_reps, in the last tile
    sizes = OnDevice(base).sizes(good["total"], good["n_runs"])

    def refused(d, what, code=_lib.GFT_E_INVALID, **kw):
        full, view, pat = d.guarded(sizes)
        rc, m, total = d.call(eng, view, good["total"], good["n_runs"], **kw)
        assert rc == code and (m, total) == (0, 0), what
        for k in NAMES:
            assert (full[k].view(torch.uint8).cpu().numpy() == pat).all(), "%s: %s was written" % (what, k)
        assert_same(OnDevice(base).run(eng), good, "after the refusal of " + what)

    for name, sp in (("order", order), ("past the end", past), ("a bad id found on the device", bad_key)):
        refused(OnDevice(base.but(name, spans=[base.spans[0], sp]), 0x3C), name)
    d = OnDevice(base)
    refused(d, "a key at or past n_keys, found on the device", key_rep=np.array([0, 1], np.uint32))
    refused(d, "an id at or past n_reps through key_rep", key_rep=np.array([0, 1, 3], np.uint32))
    refused(d, "flags", flags=1)
    refused(d, "flags, high bit", flags=0x80000000)
    refused(d, "no replacements", n_reps=0)
    refused(d, "too many replacements", n_reps=R.MAX_REPS + 1, rep_off=np.zeros(R.MAX_REPS + 2, np.uint64), rep_bytes=None)
    refused(OnDevice(base.but("long", reps=[b"", b"x" * 256, b"y"])), "a replacement of 256 bytes")
    refused(d, "rep_off[0] != 0", rep_off=np.array([1, 1, 4, 10], np.uint64))
    refused(d, "a rep_off that descends", rep_off=np.array([0, 5, 4, 10], np.uint64))
    multi = Engine(devices=[0, 0])
    try:
        refused(d, "a handle over several devices", code=_lib.GFT_E_UNSUPPORTED, handle=multi._h)
    finally:
        multi.close()
    assert d.call(eng, {}, 5)[0] == _lib.GFT_E_INVALID              # cap_bytes without an output
    # outputs that are inputs, outputs that overlap each other
    assert d.call(eng, {"run_rep": d.d_ky}, 0, d.d_ky.numel())[0] == _lib.GFT_E_INVALID
    assert d.call(eng, {"out": d.text[4:]}, 8)[0] == _lib.GFT_E_INVALID
    assert d.call(eng, {"out_off": d.d_off})[0] == _lib.GFT_E_INVALID
    both = torch.zeros(8, dtype=torch.int64, device="cuda")
    assert d.call(eng, {"out_off": both, "doc_run_off": both[1:]})[0] == _lib.GFT_E_INVALID
    # offsets that descend
    d2 = OnDevice(R.Case("two", [b"abcdef", b"ghij"], [[(1, 1)], [(1, 1)]]))
    d2.d_off = torch.tensor([0, 12, 10], dtype=torch.int64, device="cuda")
    assert d2.call(eng)[0] == _lib.GFT_E_INVALID
    d2 = OnDevice(R.Case("three", [b"abcdef", b"ghij", b"k"], [[(1, 1)], [(1, 1)], []]))
    d2.d_so = torch.tensor([0, 2, 1, 2], dtype=torch.int64, device="cuda")
    assert d2.call(eng)[0] == _lib.GFT_E_INVALID and b"span offsets descend" in L.gft_last_error(eng._h)
    # a document that would reach 4 GiB once replaced: found from the offsets alone, no text is read
    d2 = OnDevice(R.Case("big", [b"abc"], [[(1, 1)]], reps=[b"123456789"]))
    d2.d_off = torch.tensor([0, (1 << 32) - 8], dtype=torch.int64, device="cuda")
    assert d2.call(eng)[0] == _lib.GFT_E_INVALID and b"4 GiB once replaced" in L.gft_last_error(eng._h)
    # no documents: the offsets are not read; the two offset arrays get their 0
    oo = torch.full((2,), 7, dtype=torch.int64, device="cuda")
    ro = torch.full((2,), 7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert L.gft_replace_spans_device(eng._h, None, None, 0, None, None, None, None, None, 0, b"x", np.array([0, 1], np.uint64).ctypes.data, 1, 0,
                                      None, 0, oo.data_ptr(), ro.data_ptr(), None, None, None, 0, None, None) == 0
    assert oo.cpu().tolist() == [0, 7] and ro.cpu().tolist() == [0, 7]
    assert_same(OnDevice(base).run(eng), good, "after every refusal")


def test_profile_names_and_last_nonascii(eng):
    L = _lib.load()
    case = case_named("straddle_tile")
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
    for name in ("replace_runs", "replace_ids", "replace_scan", "replace_place"):
        assert eng.profile_read(name)[1] == 2, name                 # (run calls twice: count, fill)
    assert eng.profile_read("replace_copy")[1] == 1 and eng.profile_read("mark_copy")[1] == 0 and eng.profile_read("select_copy")[1] == 0
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


def as_case(name, docs, so, st, ln, key=None, reps=(b"[X]",), key_rep=None):
    so, st, ln = (t.cpu().numpy().astype(np.int64) for t in (so, st, ln))
    ky = key.cpu().numpy().astype(np.int64) if key is not None else np.zeros(st.size, np.int64)
    so = so - so[0]
    spans = [list(zip(st[so[d]:so[d + 1]].tolist(), ln[so[d]:so[d + 1]].tolist(), ky[so[d]:so[d + 1]].tolist())) for d in range(len(docs))]
    return R.Case(name, docs, spans, reps, key_rep, key is not None)


def tensors_as_result(t):
    out, out_off, doc_run_off, run_new, run_len, run_rep = t[:6]
    return {"n_runs": int(doc_run_off[-1]), "total": int(out.numel()), "out": out.cpu().numpy().tobytes(), "out_off": out_off.cpu().tolist(),
            "doc_run_off": doc_run_off.cpu().tolist(), "run_new": run_new.cpu().tolist(), "run_len": run_len.cpu().tolist(),
            "run_rep": run_rep.cpu().tolist()}


def term_ids(finder):
    L, eng = _lib.load(), finder.engine_handle()
    tp, tl = C.c_void_p(), C.c_uint32()
    ids = {}
    for t in range(int(L.gft_n_terms(eng))):
        assert L.gft_term(eng, t, C.byref(tp), C.byref(tl)) == 0
        ids[C.string_at(tp.value, tl.value)] = t
    return ids


def splice(line, spans, rep_of):
    """a line with its (start, end, keyword) hits replaced, by the reference: rep_of keyword -> (id, bytes)"""
    reps = {}
    for _, _, kw in spans:
        reps[rep_of(kw)[0]] = rep_of(kw)[1]
    table = [reps.get(k, b"") for k in range(max(reps) + 1)] if reps else [b""]
    return R.expected(R.Case("line", [line], [[(a, b - a, rep_of(kw)[0]) for a, b, kw in spans]], table))["out"]


def test_chain_spans_replace_redact_mark_excerpt_and_twice(finder):
    lines = [ln + b"\n" for ln in LOG]
    data = b"".join(lines)
    buf = resident(data)
    off, bm = finder.ProcessLinesDevice(buf, len(data))
    so, st, ln, tm, low = finder.SpansDevice(buf, off, bm)
    assert not low and int(st.numel()) > 20
    ids = term_ids(finder)
    reps = [b"[SECRET]", b"<user>", b"", b"#"]
    term_rep = np.full(len(ids), 3, np.uint32)
    term_rep[ids[b"password"]], term_rep[ids[b"root"]], term_rep[ids[b"get"]] = 0, 1, 2
    t = finder.ReplaceDevice(buf, off, so, st, ln, tm, low, False, reps, term_rep)
    case = as_case("log", lines, so, st, ln, tm, reps, term_rep.tolist())
    want = R.expected(case)
    assert_same(tensors_as_result(t), want, "split -> process -> spans -> replace")
    assert t[6] is False and want["n_runs"] > 10 and b"bad [SECRET] for <user>" in want["out"]
    # ... against the Python splice of SpansLines(source=True)
    idx, spans, _ = finder.SpansLines(data, source=True)
    by_line = dict(zip(idx.tolist(), spans))
    rep_of = lambda kw: (int(term_rep[ids[kw]]), reps[int(term_rep[ids[kw]])])  # noqa: E731
    assert want["out"] == b"".join(splice(line, by_line.get(d, []), rep_of) for d, line in enumerate(lines))
    # ... and (out, out_off, doc_run_off, run_new, run_len) is what the redaction takes: exactly the replacement bytes
    out, out_off, dro, run_new, run_len = t[:5]
    masked = out.clone()
    L = _lib.load()
    torch.cuda.synchronize()
    assert L.gft_redact_spans_device(finder.engine_handle(), masked.data_ptr(), out_off.data_ptr(), len(lines), dro.data_ptr(), run_new.data_ptr(),
                                     run_len.data_ptr(), ord("*")) == 0
    starred = [b"*" * len(r) for r in reps]
    assert masked.cpu().numpy().tobytes() == R.expected(case.but("starred", reps=starred))["out"] != want["out"]
    # ... the mark call: markers round the placeholders
    import mark as M
    docs2 = [want["out"][a:b] for a, b in zip(want["out_off"], want["out_off"][1:])]
    runs2 = [[(want["run_new"][k], want["run_len"][k]) for k in range(a, b)] for a, b in zip(want["doc_run_off"], want["doc_run_off"][1:])]
    mk = finder.MarkDevice(out, out_off, dro, run_new, run_len, False, False, b"<b>", b"</b>")
    assert mk[0].cpu().numpy().tobytes() == M.expected(M.Case("marked", docs2, runs2, b"<b>", b"</b>"))["out"]
    assert b"<b>[SECRET]</b>" in mk[0].cpu().numpy().tobytes()
    # ... the excerpt call: the text round the placeholders
    import excerpts as X
    ex = finder.ExcerptsDevice(out, out_off, dro, run_new, run_len, False, False, 6, 4, False)
    n_exc = int(ex[1].numel()) - 1
    assert n_exc > 10 and b"[SECRET]" in ex[0].cpu().numpy().tobytes() and X is not None
    eo, ed, es = ex[1].cpu().tolist(), ex[2].cpu().tolist(), ex[3].cpu().tolist()
    blob = ex[0].cpu().numpy().tobytes()
    for k in range(n_exc):
        assert blob[eo[k]:eo[k + 1]] == docs2[ed[k]][es[k]:es[k] + eo[k + 1] - eo[k]], k
    # ... and this call itself: the placeholders replaced again
    t2 = finder.ReplaceDevice(out, out_off, dro, run_new, run_len, None, False, False, [b"(again)"])
    assert_same(tensors_as_result(t2), R.expected(R.Case("twice", docs2, runs2, [b"(again)"], None, False)), "replace -> replace")


def test_chain_select_and_route_with_row_idx(finder):
    lines = [ln + b"\n" for ln in LOG]
    data = b"".join(lines)
    want_mask = finder.want_mask([0, 1])
    out, out_off, doc_idx, off, bm = finder.SelectLinesDevice(resident(data), len(data), want_mask)
    so, st, ln, tm, low = finder.SpansDevice(out, out_off, bm, want_mask, row_idx=doc_idx)
    picked = [lines[i] for i in doc_idx.cpu().tolist()]
    t = finder.ReplaceDevice(out, out_off, so, st, ln, tm, low, False, b"[X]")
    assert_same(tensors_as_result(t), R.expected(as_case("selected", picked, so, st, ln)), "process -> select -> spans -> replace")
    assert len(picked) >= 9 and int(t[2][-1]) >= len(picked)
    # a route's bucket run as the batch: doc_off[0] != 0
    out, out_off, doc_idx, bucket_doc, bucket_byte, off, bm = finder.RouteLinesDevice(resident(data), len(data), [[0], [1]])
    b0, b1 = int(bucket_doc[1]), int(bucket_doc[2])
    assert b1 > b0 > 0 and int(bucket_byte[1]) > 0
    run_off, run_idx = out_off[b0:b1 + 1].contiguous(), doc_idx[b0:b1].contiguous()
    so, st, ln, tm, low = finder.SpansDevice(out, run_off, bm, finder.want_mask([1]), row_idx=run_idx)
    picked = [lines[i] for i in run_idx.cpu().tolist()]
    t = finder.ReplaceDevice(out, run_off, so, st, ln, tm, low, False, b"")
    assert_same(tensors_as_result(t), R.expected(as_case("bucket", picked, so, st, ln, reps=[b""])), "a route's bucket run")


def test_replace_lines_with_bytes_and_with_a_dict(finder):
    lines = [ln + b"\n" for ln in LOG]
    data = b"".join(lines)
    idx, spans, _ = finder.SpansLines(data, source=True)
    by_line = dict(zip(idx.tolist(), spans))
    got, low = finder.ReplaceLines(data)
    assert not low and got == b"".join(splice(line, by_line.get(d, []), lambda kw: (0, b"[REDACTED]")) for d, line in enumerate(lines))
    assert b"bad [REDACTED] for [REDACTED]" in got
    got, _ = finder.ReplaceLines(data, b"")
    assert got == b"".join(splice(line, by_line.get(d, []), lambda kw: (0, b"")) for d, line in enumerate(lines))
    # a dict: insertion order is the priority, None the default; a keyword given in upper case finds the lowered term
    with_ = {"root": b"<user>", b"PASSWORD": b"[SECRET]", "oom": b"<user>", None: b"?"}
    table = {b"root": (0, b"<user>"), b"password": (1, b"[SECRET]"), b"oom": (0, b"<user>")}
    got, _ = finder.ReplaceLines(data, with_)
    assert got == b"".join(splice(line, by_line.get(d, []), lambda kw: table.get(kw, (2, b"?"))) for d, line in enumerate(lines))
    assert b"bad [SECRET] for <user>" in got and b"? /admin ?" in got
    # without the key None the default is [REDACTED]
    got, _ = finder.ReplaceLines(data, {"root": b"<user>"})
    assert b"bad [REDACTED] for <user>" in got
    with pytest.raises(ValueError):
        finder.ReplaceLines(data, {"nosuchkeyword": b"x"})


def test_replace_lines_of_a_lowered_batch(finder):
    lines = [ln + b"\n" for ln in LOG]
    lines[2] = "GET /café 403 ÿ\n".encode()
    lines[3] = "KERNEL: OOM-killer invoked by CAFÉ\n".encode()
    data = b"".join(lines)
    with_ = {"café": "«bar»".encode(), "oom": b"[MEM]", None: b"[R]"}
    table = {"café".encode(): (0, "«bar»".encode()), b"oom": (1, b"[MEM]")}
    for source in (True, False):
        idx, spans, low = finder.SpansLines(data, source=source)
        got, glow = finder.ReplaceLines(data, with_, source=source)
        assert low and glow
        by_line = dict(zip(idx.tolist(), spans))
        texts = lines if source else [ln.decode().lower().encode() for ln in lines]
        assert got == b"".join(splice(t, by_line.get(d, []), lambda kw: table.get(kw, (2, b"[R]"))) for d, t in enumerate(texts)), source
        got.decode("utf-8")                                          # valid UTF-8 stays valid
        assert ("invoked by «bar»".encode() in got) and (b"KERNEL: [MEM]-killer" in got) == source


def test_replace_lines_with_whole_words():
    f = Finder(GpuEngine.__new__(GpuEngine), EmptyRgxEngine(), False, whole_words=True)
    try:
        f.AddExpressions(['"he" or "cat"'])
        got, _ = f.ReplaceLines(b"ushers he concatenate cat\nthe cat\n", {"he": b"[HE]", "cat": b""})
        assert got == b"ushers [HE] concatenate \nthe \n"
        f.whole_words = False
        got, _ = f.ReplaceLines(b"ushers he cat\n", {"he": b"[HE]", "cat": b""})
        assert got == b"us[HE]rs [HE] \n"
    finally:
        f.close()
