"""Excerpts snapped to word or line borders on the device (the <true> instantiation of k_excerpt_window, csrc/gft_excerpt.hip):
gft_excerpt_spans_snap_device bit for bit against the reference of snap_cases.py on every fixed case and the random batches, the
text at sixteen alignments, the lead bytes, the slack and the allocations round every output filled with 0x00, 0xBF or 'a' (a
word byte: a walk that left its document would go on); the cap protocol; no snap bit = gft_excerpt_spans_device on the same
handle; the refusals, which leave the handle usable; Finder.ExcerptLines(snap=) on the records of examples/snippet_quickstart.py,
over a batch that leaves ASCII in both forms, with mark=, and behind a whole-word finder.  All comparisons are exact."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch  # noqa: F401  (before libgft.so is loaded: one HIP runtime)

import excerpts as X
import snap_cases as S
from gofindthem_amd import _lib
from gofindthem_amd.engine import Engine, excerpt_shape
from gofindthem_amd.finder import EmptyRgxEngine, Finder, GpuEngine

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE, TRIP = excerpt_shape()
FIXED = S.fixed_cases(TILE)
G = 8                                                               # guard entries on either side of every output
NAMES = ("out", "exc_off", "exc_doc", "exc_start", "exc_span_off", "span_rel", "doc_exc_off")
DTYPES = {"out": torch.uint8, "exc_off": torch.int64, "exc_doc": torch.int64, "exc_start": torch.int32, "exc_span_off": torch.int64,
          "span_rel": torch.int32, "doc_exc_off": torch.int64}
FILLS = (0x00, 0xBF, ord("a"))


@pytest.fixture(scope="module")
def eng():
    e = Engine()
    yield e
    e.close()


_REF = {}


def reference(case):
    if case.name not in _REF:
        _REF[case.name] = S.expected(case)
    return _REF[case.name]


class OnDevice:
    """a case on the device: the text `at` bytes into an allocation whose every other byte -- in front, the lead, the 64 bytes of
    slack -- holds `fill`; the span arrays behind span_lead entries no call may read"""

    def __init__(self, case, fill=0x00, at=0, span_lead=0, span_tail=0):
        self.case, self.fill = case, fill
        self.blob, self.off, self.so, self.st, self.ln = case.arrays(fill, span_lead, span_tail)
        buf = torch.full((at + self.blob.size + 64,), fill, dtype=torch.uint8, device="cuda")
        if self.blob.size:
            buf[at:at + self.blob.size] = torch.from_numpy(self.blob.copy()).cuda()
        self.text = buf[at:]
        self.n = len(case.docs)
        self.d_off = torch.from_numpy(self.off.astype(np.int64)).cuda()
        self.d_so = torch.from_numpy(self.so.astype(np.int64)).cuda()
        self.d_st = torch.from_numpy(self.st.view(np.int32).copy()).cuda()
        self.d_ln = torch.from_numpy(self.ln.view(np.int32).copy()).cuda()

    def call(self, e, outs=None, cap_bytes=0, cap_exc=0, flags=None, reach=None, plain=False, handle=None):
        """the raw call -> (rc, n_exc, total); outs: name -> tensor.  plain: gft_excerpt_spans_device"""
        outs = outs or {}
        m, total = C.c_uint64(0), C.c_uint64(0)
        p = {k: (outs[k].data_ptr() if outs.get(k) is not None else None) for k in NAMES}
        c = self.case
        head = (handle or e._h, self.text.data_ptr(), self.d_off.data_ptr(), self.n, self.d_so.data_ptr(), self.d_st.data_ptr() if self.st.size else None,
                self.d_ln.data_ptr() if self.ln.size else None, c.before, c.after, c.flags if flags is None else flags)
        tail = (p["out"], cap_bytes, p["exc_off"], p["exc_doc"], p["exc_start"], p["exc_span_off"], cap_exc, p["span_rel"], p["doc_exc_off"],
                C.byref(m), C.byref(total))
        torch.cuda.synchronize()
        L = _lib.load()
        rc = L.gft_excerpt_spans_device(*head, *tail) if plain else L.gft_excerpt_spans_snap_device(*head, c.reach if reach is None else reach, *tail)
        return rc, int(m.value), int(total.value)

    def sizes(self, m, total):
        return {"out": total, "exc_off": m + 1, "exc_doc": m, "exc_start": m, "exc_span_off": m + 1, "span_rel": self.st.size, "doc_exc_off": self.n + 1}

    def guarded(self, sizes, shift=0):
        full, view = {}, {}
        pat = 0x5A if self.fill == 0 else self.fill
        for k, n in sizes.items():
            extra = shift if k == "out" else 0
            t = torch.empty(n + 2 * G + extra, dtype=DTYPES[k], device="cuda")
            t.view(torch.uint8).fill_(pat)
            full[k], view[k] = t, t[G + extra:G + extra + n]
        return full, view, pat

    def run(self, e, cap_bytes=None, cap_exc=None, shift=0, **kw):
        """count, then fill guarded tensors -> a dict like the reference's, arrays cut to what the caps allow; the guards compared"""
        rc, m, total = self.call(e, **kw)
        assert rc == 0, _lib.load().gft_last_error(e._h)
        cb = total if cap_bytes is None else cap_bytes
        ce = m if cap_exc is None else cap_exc
        sizes = self.sizes(min(m, ce), min(total, cb))
        sizes["exc_off"] = sizes["exc_span_off"] = min(m, ce) + 1
        full, view, pat = self.guarded(sizes, shift)
        rc, m2, total2 = self.call(e, view, cb, ce, **kw)
        assert rc == 0 and (m2, total2) == (m, total), _lib.load().gft_last_error(e._h)
        got = {"n_exc": m, "total": total}
        for k in NAMES:
            raw = full[k].view(torch.uint8).cpu().numpy()
            item = full[k].element_size()
            extra = shift if k == "out" else 0
            lo, hi = (G + extra) * item, (G + extra + sizes[k]) * item
            assert (raw[:lo] == pat).all() and (raw[hi:] == pat).all(), "%s: a store outside the output" % k
            got[k] = view[k].cpu().numpy()
        got["out"] = got["out"].tobytes()
        return got


def assert_same(got, want, what, untouched=None):
    diff = X.same(got, want, untouched)
    assert diff is None, "%s: %s" % (what, diff)


def test_symbols():
    L = _lib.load()
    for name in ("gft_excerpt_spans_snap_device", "gft_finder_excerpts_snap_device"):
        assert hasattr(L, name)


@pytest.mark.parametrize("i", range(len(FIXED)), ids=[c.name for c in FIXED])
def test_fixed_case_at_sixteen_alignments(eng, i):
    case = FIXED[i]
    want = reference(case)
    for at in range(16):
        fill = FILLS[(at + i) % 3]
        assert_same(OnDevice(case, fill, at).run(eng, shift=(at * 5) % 16), want, "%s, fill %#x, text at +%d" % (case.name, fill, at))


def test_fixed_cases_behind_a_span_base(eng):
    for j, case in enumerate(S.small(FIXED)[::3]):
        fill = FILLS[j % 3]
        d = OnDevice(case, fill, j % 16, 3, 2)
        pat = 0x5A if fill == 0 else fill
        assert_same(d.run(eng), S.expected(case, None, 3, 2), case.name, untouched=int(np.array([pat] * 4, np.uint8).view(np.int32)[0]))


def test_random_batches(eng):
    for j, case in enumerate(S.random_cases()):
        want = reference(case)
        for at in (0, 5, 11):
            assert_same(OnDevice(case, ord("a"), at).run(eng, shift=at), want, "%s at +%d" % (case.name, at))


def test_cap_protocol(eng):
    case = next(c for c in FIXED if c.name == "exactly the hit lines, adjacent lines apart")
    want = reference(case)
    m, total = want["n_exc"], want["total"]
    assert m >= 4
    d = OnDevice(case, 0xBF, 3)
    assert d.call(eng) == (0, m, total)                              # count only
    assert_same(d.run(eng, total, m), want, "exact caps")
    got = d.run(eng, cap_exc=m - 1)                                  # one entry short: nothing at or past the cap (run compares the guards)
    assert got["exc_off"].tolist() == want["exc_off"][:m] and got["exc_span_off"].tolist() == want["exc_span_off"][:m]
    assert got["exc_doc"].tolist() == want["exc_doc"][:m - 1] and got["exc_start"].tolist() == want["exc_start"][:m - 1]
    assert got["span_rel"].tolist() == want["span_rel"] and got["doc_exc_off"].tolist() == want["doc_exc_off"] and got["out"] == want["out"]
    for cb in (want["exc_off"][1] + 7, want["exc_off"][2], 1):      # a cap that cuts an excerpt, one on a border, one byte
        got = d.run(eng, cap_bytes=cb, shift=5)
        assert got["out"] == want["out"][:cb] and got["exc_off"].tolist() == want["exc_off"], cb
    big = next(c for c in FIXED if c.name.startswith("reach 4096, a word 4096"))
    want = reference(big)
    assert want["n_exc"] == 1 and want["total"] == S.REACH_MAX + 1
    got = OnDevice(big, ord("a"), 7).run(eng, cap_bytes=4000, shift=3)
    assert got["out"] == want["out"][:4000]


def test_no_snap_bit_is_the_plain_call(eng):
    """flags without a snap bit, whatever the reach: the old entry point's answer on the same handle, an old call before and after"""
    T, K = excerpt_shape()
    names = ("gap 0", "rune snap 2/3", "a run crosses a tile border", "one excerpt past the copy's tile", "windows touch in the blob")
    for name in names:
        xc = next(c for c in X.fixed_cases(T, K) if c.name == name)
        case = S.Case(xc.name, xc.docs, xc.spans, xc.before, xc.after, None, 64, xc.runes, xc.lead)
        d = OnDevice(case, 0xBF, 5)
        before = d.run(eng, plain=True)
        for reach in (0, 64, S.REACH_MAX):
            assert_same(d.run(eng, reach=reach), before, "%s, reach %d" % (name, reach))
        assert_same(d.run(eng, plain=True), before, name + ", the plain call again")
        assert_same(before, X.expected(xc), name)
    # a snapped call between two plain ones changes neither
    sc = next(c for c in FIXED if c.name == "one byte apart, touching after the snap")
    plain_case = sc.but("plain", snap=None)
    a = OnDevice(plain_case).run(eng, plain=True)
    assert_same(OnDevice(sc).run(eng), reference(sc), sc.name)
    assert_same(OnDevice(plain_case).run(eng, plain=True), a, "the plain call behind a snapped one")
    assert a["n_exc"] == 2 and reference(sc)["n_exc"] == 1


def test_refusals_leave_the_handle_usable(eng):
    L = _lib.load()
    case = next(c for c in FIXED if c.name == "one word apart")
    good = reference(case)
    d = OnDevice(case, ord("a"))
    full, view, pat = d.guarded(d.sizes(good["n_exc"], good["total"]))
    for flags, reach in ((S.WORDS | S.LINES, 1), (S.WORDS | S.LINES | S.RUNES, 0), (8, 1), (0x80000002, 1), (S.WORDS, S.REACH_MAX + 1),
                         (S.LINES, 0xFFFFFFFF), (0, S.REACH_MAX + 1)):
        rc, m, total = d.call(eng, view, good["total"], good["n_exc"], flags=flags, reach=reach)
        assert rc == _lib.GFT_E_INVALID and (m, total) == (0, 0), (flags, reach)
        assert b"gft_excerpt_spans_snap_device" in L.gft_last_error(eng._h)
    for k in NAMES:
        assert (full[k].view(torch.uint8).cpu().numpy() == pat).all(), "%s was written" % k
    assert d.call(eng, flags=S.WORDS, plain=True)[0] == _lib.GFT_E_INVALID          # the plain call knows one flag alone
    assert d.call(eng, flags=S.LINES, plain=True)[0] == _lib.GFT_E_INVALID
    # the plain call's refusals are the snapped call's: a span past its document's end, outputs that are inputs, several devices
    bad = OnDevice(case.but("past the end", spans=[[(len(case.docs[0]), 1)]]), ord("a"))
    rc, m, total = bad.call(eng, view, good["total"], good["n_exc"])
    assert rc == _lib.GFT_E_INVALID and (m, total) == (0, 0)
    for k in NAMES:
        assert (full[k].view(torch.uint8).cpu().numpy() == pat).all(), "%s was written" % k
    assert d.call(eng, {"span_rel": d.d_st})[0] == _lib.GFT_E_INVALID
    assert d.call(eng, {}, 5, 0)[0] == _lib.GFT_E_INVALID
    multi = Engine(devices=[0, 0])
    try:
        assert d.call(eng, handle=multi._h)[0] == _lib.GFT_E_UNSUPPORTED
    finally:
        multi.close()
    assert_same(d.run(eng), good, "after every refusal")


def test_engine_wrapper_and_profile_names(eng):
    case = next(c for c in FIXED if c.name == "exactly the hit lines, adjacent lines apart")
    d = OnDevice(case)
    eng.profile(True)
    eng.profile_reset()
    t = eng.excerpt_spans_device(d.text, d.d_off, d.d_so, d.d_st, d.d_ln, 0, 0, False, snap="lines", reach=S.REACH_MAX)
    for name in ("excerpt_window", "excerpt_smin", "excerpt_scan", "excerpt_place"):
        assert eng.profile_read(name)[1] == 2, name
    assert eng.profile_read("excerpt_copy")[1] == 1
    eng.profile(False)
    want = reference(case)
    assert t[0].cpu().numpy().tobytes() == want["out"] and t[1].cpu().tolist() == want["exc_off"] and t[3].cpu().tolist() == want["exc_start"]
    with pytest.raises(ValueError):
        eng.excerpt_spans_device(d.text, d.d_off, d.d_so, d.d_st, d.d_ln, snap="sentences")


# ---- the finder -----------------------------------------------------------------------------------------------------------------
def example():
    spec = importlib.util.spec_from_file_location("snippet_quickstart", os.path.join(ROOT, "examples", "snippet_quickstart.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def finder():
    f = Finder(GpuEngine.__new__(GpuEngine), EmptyRgxEngine(), False)
    f.AddExpressions(example().EXPRESSIONS)
    yield f
    f.close()


def lines_against_the_reference(f, data, lines_cut_from, snap, reach, before, after, source):
    """ExcerptLines(snap=) against the reference over the spans SpansLines reports; lines_cut_from: the lines the excerpts are cut
    from (the caller's, or their lower-case form).  Returns the excerpts"""
    sidx, sspans, _ = f.SpansLines(data, source=source)
    idx, exc, low = f.ExcerptLines(data, before=before, after=after, source=source, snap=snap, reach=reach)
    assert idx.tolist() == sidx.tolist()
    for d, per_line, sp in zip(idx.tolist(), exc, sspans):
        line = lines_cut_from[d]
        want = S.expected(S.Case("line", [line], [[(a, b - a) for a, b, _ in sp]], before, after, snap, reach, runes=True))
        texts = [want["out"][a:b] for a, b in zip(want["exc_off"], want["exc_off"][1:])]
        assert [(s, t) for s, t, _ in per_line] == list(zip(want["exc_start"], texts)), (d, snap)
        hits = [(s + a, s + b, kw) for s, _, h in per_line for a, b, kw in h]
        assert hits == sp, d
    return idx, exc, low


def test_excerpt_lines_of_the_example_records(finder):
    mod = example()
    data = b"\n".join(mod.RECORDS) + b"\n"
    lines = data.split(b"\n")[:-1]
    lines = [ln + b"\n" for ln in lines]
    # ... which leave ASCII: source=True cuts the caller's bytes, source=False their lower-case form
    lowered = [ln.decode().lower().encode() for ln in lines]
    assert lowered != lines and [len(a) for a in lowered] == [len(b) for b in lines]
    for snap, reach in (("words", 64), ("words", 3), ("lines", 4096), ("lines", 10)):
        _, exc, low = lines_against_the_reference(finder, data, lines, snap, reach, 12, 12, True)
        assert low and any(exc)
        _, exc2, low2 = lines_against_the_reference(finder, data, lowered, snap, reach, 12, 12, False)
        assert low2 and exc2 != exc
    # the lines the hits stand in, without their newline
    idx, exc, _ = finder.ExcerptLines(data, before=0, after=0, snap="lines", reach=4096)
    assert [[(s, t) for s, t, _ in per_line] for per_line in exc] == [[(0, lines[d][:-1])] for d in idx.tolist()]
    # word borders: no excerpt of reach 64 begins or ends inside a word of its line
    idx, exc, _ = finder.ExcerptLines(data, before=12, after=12, snap="words", reach=64)
    seen = 0
    for d, per_line in zip(idx.tolist(), exc):
        for s, t, _ in per_line:
            assert not S.cuts_word(lines[d], s) and not S.cuts_word(lines[d], s + len(t)), (d, s, t)
            seen += 1
    plain = finder.ExcerptLines(data, before=12, after=12)[1]
    assert seen >= 4 and plain != exc
    # the multi-line records themselves, the example's way: the third form is exactly the hit lines
    found = mod.snippets(finder, mod.RECORDS, before=0, after=0, snap="lines", reach=4096)
    assert [t for _, t in found[0]] == [b"failed to authenticate user administrator from 10.0.0.7"]
    assert found[1] == [] and [t for _, t in found[2]] == [b"upstream timeout after 30 s", b"bad password for root"]
    assert [t for _, t in found[3]] == ["CAFÉ gateway: PASSWORD expired for josé".encode()]
    words = mod.snippets(finder, mod.RECORDS, before=12, after=12, snap="words", reach=64)
    raw = mod.snippets(finder, mod.RECORDS, before=12, after=12)
    assert words != raw
    for d, (ws, rs) in enumerate(zip(words, raw)):
        assert len(ws) <= len(rs)
        for s, t in ws:
            assert mod.RECORDS[d][s:s + len(t)] == t and not S.cuts_word(mod.RECORDS[d], s) and not S.cuts_word(mod.RECORDS[d], s + len(t))


def test_excerpt_lines_snapped_and_marked(finder):
    data = b"\n".join(example().RECORDS) + b"\n"
    for snap in ("words", "lines"):
        idx, exc, _ = finder.ExcerptLines(data, before=5, after=5, snap=snap, reach=64)
        midx, mexc, _ = finder.ExcerptLines(data, before=5, after=5, snap=snap, reach=64, mark=(b"[", b"]"))
        assert midx.tolist() == idx.tolist() and any(exc)
        for per_line, marked in zip(exc, mexc):
            assert [s for s, _, _ in per_line] == [s for s, _, _ in marked]
            for (_, text, hits), (_, mtext, mhits) in zip(per_line, marked):
                assert mtext.replace(b"[", b"").replace(b"]", b"") == text and mtext.count(b"[") == mtext.count(b"]") >= 1
                assert [mtext[a:b] for a, b, _ in mhits] == [text[a:b] for a, b, _ in hits]


def test_whole_word_finder_with_the_word_snap():
    f = Finder(GpuEngine.__new__(GpuEngine), EmptyRgxEngine(), False, whole_words=True)
    try:
        f.AddExpressions(['"he"', '"user"', '"administrator_of_the_whole_wide_world"'])
        lines = [b"ushers he she hers\n", b"the user-name of he: user_7, (he) and the superuser\n", b"he\n", b"\n",
                 b"say he administrator_of_the_whole_wide_worlds\n", "naïve he—she, hé he\n".encode()]
        data = b"".join(lines)
        reach = 12
        sidx, sspans, _ = f.SpansLines(data, source=True)
        idx, exc, _ = f.ExcerptLines(data, before=4, after=4, snap="words", reach=reach)
        assert idx.tolist() == sidx.tolist() == [0, 1, 2, 4, 5]
        gave_up = 0
        for d, per_line, sp in zip(idx.tolist(), exc, sspans):
            line = lines[d]

            def ref(r):
                w = S.expected(S.Case("line", [line], [[(a, b - a) for a, b, _ in sp]], 4, 4, "words", r, runes=True))
                return [(s, w["out"][a:b]) for s, a, b in zip(w["exc_start"], w["exc_off"], w["exc_off"][1:])]
            assert [(s, t) for s, t, _ in per_line] == ref(reach), d
            far = {e for s, t in ref(S.REACH_MAX) for e in (s, s + len(t))}
            for s, t, hits in per_line:
                assert hits, (d, s)
                for edge in (s, s + len(t)):
                    if S.cuts_word(line, edge):
                        # only where the reference says the walk gave up: with all the reach there is, no excerpt has an edge here
                        assert edge not in far, (d, edge)
                        gave_up += 1
        assert gave_up >= 1
    finally:
        f.close()
