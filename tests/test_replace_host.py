"""Replace on the host: gft_debug_replace_spans -- the runs by the excerpt's walk, the copy tile by tile, trip by trip and lane by
lane through the header the kernels compile -- against the reference of replace.py, written from the contract alone, on every
fixed case, the span counts round the walk's borders and the random batches; its runs against gft_debug_mark_spans of the same
input; both caps into guarded arrays, every output NULL on its own, the refusals, which must leave every output untouched, and
the identities.  All comparisons are exact; no device needed."""
import ctypes as C

import numpy as np
import pytest

import replace as R
from gofindthem_amd import _lib
from gofindthem_amd.engine import GftError, mark_spans_host, replace_shape, replace_spans_host, replace_table

TILE_SPANS, TRIP_TILES, CHUNK, TILE, WINDOW, LDS_TABLE = replace_shape()
GUARD = 3
NAMES = ("out", "out_off", "doc_run_off", "run_new", "run_len", "run_rep")
PER_RUN = ("run_new", "run_len", "run_rep")


def run(case, fill=0x00, span_lead=0, span_tail=0, **kw):
    blob, off, so, st, ln, ky = case.arrays(fill, span_lead, span_tail)
    return replace_spans_host(blob, off, so, st, ln, case.reps, ky, case.key_rep if case.keyed else None, **kw)


def cut(r, case, guard=0, cap=None, cap_runs=None):
    """the arrays of a result, cut to their sizes; the guard entries must hold their pattern"""
    total = r["total"] if cap is None else min(cap, r["total"])
    runs = r["n_runs"] if cap_runs is None else min(cap_runs, r["n_runs"])
    sizes = {"out": total, "out_off": len(case.docs) + 1, "doc_run_off": len(case.docs) + 1, "run_new": runs, "run_len": runs, "run_rep": runs}
    got = {"n_runs": r["n_runs"], "total": r["total"]}
    for k in NAMES:
        v = r[k]
        if v is None:
            got[k] = [] if k != "out" else b""
            continue
        got[k] = v[:sizes[k]].tolist()
        tail = v[sizes[k]:]
        assert tail.size >= guard and (tail.view(np.uint8) == 0xA5).all(), "%s: a store behind the cap" % k
    got["out"] = bytes(got["out"])
    return got


def case_named(name):
    return next(c for c in FIXED if c.name == name)


def test_symbols_present():
    L = _lib.load()
    names = ("gft_replace_spans_device", "gft_debug_replace_spans", "gft_debug_replace_shape", "gft_finder_replace_device")
    for name in names:
        assert hasattr(L, name) and name in _lib.SYMBOLS
    assert replace_shape()[:4] == (256, 1024, 16, 4096) and (R.CHUNK, R.TILE, R.TRIP) == (16, 4096, 1024)
    header = open(_lib.__file__.replace("gofindthem_amd/_lib.py", "include/gft.h")).read()
    for name in names + ("GFT_REPLACE_MAX 255u",):
        assert name in header


def test_the_cases_tell_the_mutants_apart():
    assert R.assert_not_vacuous()


FIXED = R.fixed_cases()


@pytest.mark.parametrize("i", range(len(FIXED)), ids=[c.name for c in FIXED])
def test_fixed_case(i):
    case = FIXED[i]
    want = R.expected(case)
    for fill in (0x00, (b"".join(case.reps) + b"<")[0]):
        for shift in (0, 1 + i % 15):
            assert R.same(cut(run(case, fill, guard=GUARD, shift=shift), case, GUARD), want), "%s, lead bytes %#x, out at +%d" % (case.name, fill, shift)


def test_fixed_cases_behind_a_span_base():
    """span_off[0] != 0, with entries on both sides that every call would refuse if it read them"""
    for case in FIXED:
        if case.name == "table_65536":
            continue                                                # (its table is what it is about: test_fixed_case has it)
        assert R.same(cut(run(case, 0x3C, 3, 2, guard=GUARD, shift=7), case, GUARD), R.expected(case, None, 3)), case.name


COUNTS = R.count_cases(TILE_SPANS, TRIP_TILES)


@pytest.mark.parametrize("i", range(len(COUNTS)), ids=[c.name for c in COUNTS])
def test_span_counts_round_the_walks_borders(i):
    case = COUNTS[i]
    assert R.same(cut(run(case, 0x3C, guard=GUARD, shift=9), case, GUARD), R.expected(case)), case.name


def test_random_batches():
    for seed in (1, 2, 3):
        for case in R.random_cases(seed):
            assert R.same(cut(run(case, 0xEE, guard=GUARD, shift=case.lead % 16), case, GUARD), R.expected(case)), case.name


def test_runs_are_the_highlights_runs():
    for case in FIXED + R.random_cases(4) + COUNTS[:3]:
        blob, off, so, st, ln, _ = case.arrays()
        r = run(case)
        m = mark_spans_host(blob, off, so, st, ln, b"<", b">")
        assert r["n_runs"] == m["n_runs"] and r["doc_run_off"].tolist() == m["doc_run_off"].tolist(), case.name
        # every run's replacement stands in the replaced text at the place the index arrays say
        out = bytes(r["out"][:r["total"]].tolist()) if r["out"] is not None else b""
        for d in range(len(case.docs)):
            for k in range(int(r["doc_run_off"][d]), int(r["doc_run_off"][d + 1])):
                at = int(r["out_off"][d]) + int(r["run_new"][k])
                assert out[at:at + int(r["run_len"][k])] == case.reps[int(r["run_rep"][k])], (case.name, k)


def test_cap_protocol():
    case = case_named("straddle_tile")
    want = R.expected(case)
    total, runs = want["total"], want["n_runs"]
    assert run(case, count_only=True) == {"n_runs": runs, "total": total}
    o = TILE - 2
    assert want["out"][o:o + 6] == b"[NAME]" and runs == 2
    # 0, 1, inside text, inside a replacement, at its ends, exact, and room to spare
    for cb in (0, 1, 100, o, o + 2, o + 5, o + 6, TILE, total - 1, total, total + 5):
        for cr in (0, 1, 2, 4):
            for shift in (0, 5):
                r = run(case, 0x3C, cap_bytes=cb, cap_runs=cr, guard=GUARD, shift=shift)
                if cb > total:                                      # (room to spare stays as it was)
                    assert (r["out"][total:] == 0xA5).all()
                    r["out"] = r["out"][:total + GUARD]
                got = cut(r, case, GUARD, cb, cr)
                assert got["out"] == want["out"][:cb], (cb, cr)
                assert got["out_off"] == want["out_off"] and got["doc_run_off"] == want["doc_run_off"]
                assert all(got[k] == want[k][:cr] for k in PER_RUN), (cb, cr)
                assert (got["n_runs"], got["total"]) == (runs, total)


@pytest.mark.parametrize("name", NAMES)
def test_every_output_null_on_its_own(name):
    for case in (case_named("touch_across_docs"), case_named("empty_docs"), case_named("key_rep_given")):
        want = R.expected(case)
        r = run(case, omit=(name,), guard=GUARD, cap_bytes=0 if name == "out" else None)
        assert r[name] is None
        got = cut(r, case, GUARD, 0 if name == "out" else None)
        for k in NAMES:
            if k != name:
                assert got[k] == want[k], k


def test_refusals_leave_every_output_untouched():
    L = _lib.load()
    base = COUNTS[2]
    spans1 = list(base.spans[1])
    order = spans1[:-2] + [spans1[-1], spans1[-2]]
    past = spans1[:-1] + [(spans1[-1][0], len(base.docs[1]), 0)]
    want = R.expected(base)
    total, runs = want["total"], want["n_runs"]
    big = 0xA5A5A5A5A5A5A5A5

    def refused(case, what, **kw):
        blob, off, so, st, ln, ky = case.arrays()
        rep_bytes, rep_off = replace_table(case.reps)
        n_reps = kw.get("n_reps", rep_off.size - 1)
        rep_off = kw.get("rep_off", rep_off)
        kr = kw.get("key_rep")
        outs = [np.full(total, 0xA5, np.uint8), np.full(len(case.docs) + 1, big, np.uint64), np.full(len(case.docs) + 1, big, np.uint64)]
        outs += [np.full(runs, 0xA5A5A5A5, np.uint32) for _ in range(3)]
        n_runs, n_bytes = C.c_uint64(77), C.c_uint64(77)
        rc = L.gft_debug_replace_spans(blob.ctypes.data, kw.get("off", off).ctypes.data, len(case.docs), kw.get("so", so).ctypes.data, st.ctypes.data,
                                       ln.ctypes.data, kw.get("ky", ky).ctypes.data, kr.ctypes.data if kr is not None else None,
                                       kr.size if kr is not None else 0, kw.get("rep_bytes", rep_bytes), rep_off.ctypes.data, n_reps,
                                       kw.get("flags", 0), outs[0].ctypes.data, total, outs[1].ctypes.data, outs[2].ctypes.data, outs[3].ctypes.data,
                                       outs[4].ctypes.data, outs[5].ctypes.data, runs, C.byref(n_runs), C.byref(n_bytes))
        assert rc == _lib.GFT_E_INVALID, what
        assert (n_runs.value, n_bytes.value) == (0, 0), what
        for a in outs:
            assert (a.view(np.uint8) == 0xA5).all(), what

    refused(base.but("order", spans=[base.spans[0], order]), "ends that descend")
    refused(base.but("past", spans=[base.spans[0], past]), "a span past its document")
    refused(base, "flags", flags=1)
    refused(base, "no replacements", n_reps=0)
    refused(base, "too many replacements", n_reps=R.MAX_REPS + 1, rep_off=np.zeros(R.MAX_REPS + 2, np.uint64), rep_bytes=None)
    refused(base.but("long", reps=[b"", b"x" * 256, b"y"]), "a replacement of 256 bytes")
    refused(base, "rep_off[0] != 0", rep_off=np.array([1, 1, 4, 10], np.uint64))
    refused(base, "a rep_off that descends", rep_off=np.array([0, 5, 4, 10], np.uint64))
    refused(base.but("id", reps=[b"a", b"b"]), "an id at or past n_reps")
    refused(base, "a key at or past n_keys", key_rep=np.array([0, 1], np.uint32))
    refused(base, "an id at or past n_reps through key_rep", key_rep=np.array([0, 1, 3], np.uint32))
    _, off, so, _, _, _ = base.arrays()
    bad_off = off.copy()
    bad_off[1] = bad_off[2] + 1
    refused(base, "document offsets that descend", off=bad_off)
    bad_so = so.copy()
    bad_so[1] = bad_so[2] + 1
    refused(base, "span offsets that descend", so=bad_so)
    # a document that would reach 4 GiB once replaced: found from the offsets alone, no text is read
    one = R.Case("big", [b"abc"], [[(1, 1)]], reps=[b"123456789"])
    refused(one, "a document that reaches 4 GiB once replaced", off=np.array([0, (1 << 32) - 8], np.uint64))
    refused(one, "a document of 4 GiB", off=np.array([0, 1 << 32], np.uint64))
    # an output that is an input
    blob, off, so, st, ln, ky = base.arrays()
    ky = ky.copy()
    rep_bytes, rep_off = replace_table(base.reps)
    rc = L.gft_debug_replace_spans(blob.ctypes.data, off.ctypes.data, 2, so.ctypes.data, st.ctypes.data, ln.ctypes.data, ky.ctypes.data, None, 0,
                                   rep_bytes, rep_off.ctypes.data, 3, 0, None, 0, None, None, None, None, ky.ctypes.data, ky.size, None, None)
    assert rc == _lib.GFT_E_INVALID and ky.tolist() == base.arrays()[5].tolist()
    with pytest.raises(GftError):
        run(base, flags=2)
    # no documents: the offsets are not read; the two offset arrays get their 0
    oo, ro = np.full(2, 7, np.uint64), np.full(2, 7, np.uint64)
    assert L.gft_debug_replace_spans(None, None, 0, None, None, None, None, None, 0, b"x", np.array([0, 1], np.uint64).ctypes.data, 1, 0, None, 0,
                                     oo.ctypes.data, ro.ctypes.data, None, None, None, 0, None, None) == 0
    assert oo.tolist() == [0, 7] and ro.tolist() == [0, 7]


def test_identities():
    from gofindthem_amd.engine import redact_spans_host
    for case in FIXED[9:] + R.random_cases(5, 20):
        blob, off, so, st, ln, ky = case.arrays()
        text = b"".join(case.docs)
        # no spans: the text
        r = replace_spans_host(blob, off, np.zeros(len(case.docs) + 1, np.uint64), [], [], case.reps)
        assert r["n_runs"] == 0 and (bytes(r["out"].tolist()) if r["out"] is not None else b"") == text, case.name
        # replacements equal to the runs' own bytes: the text.  One table entry per run, asked for through the keys
        want = R.expected(case)
        m = mark_spans_host(blob, off, so, st, ln, b"", b"")
        own, keys = [], np.zeros(st.size, np.uint32)
        for d, (doc, spans, ids) in enumerate(zip(case.docs, case.spans, case.ids())):
            comps = R.runs_of(spans, ids)
            for k, (a, n, _) in enumerate(spans):
                j = max(i for i, (S, _, _) in enumerate(comps) if S <= a)
                keys[int(so[d]) + k] = len(own) + j
            own += [doc[S:E] for S, E, _ in comps]
        if own and max(len(o) for o in own) <= R.REPLACE_MAX:
            r = replace_spans_host(blob, off, so, st, ln, own, keys)
            assert r["n_runs"] == m["n_runs"] == len(own) and bytes(r["out"].tolist() if r["out"] is not None else b"") == text, case.name
        # the redaction over the handed-back run list masks exactly the replacement bytes
        r = run(case)
        if r["out"] is None:
            continue
        out = bytes(r["out"].tolist())
        red = redact_spans_host(r["out"].copy(), r["out_off"], r["doc_run_off"], r["run_new"] if r["run_new"] is not None else [],
                                r["run_len"] if r["run_len"] is not None else [], 0)
        exp = bytearray(out)
        for d in range(len(case.docs)):
            for k in range(want["doc_run_off"][d], want["doc_run_off"][d + 1]):
                at = want["out_off"][d] + want["run_new"][k]
                exp[at:at + want["run_len"][k]] = b"\x00" * want["run_len"][k]
        assert bytes(np.asarray(red).tolist()) == bytes(exp), case.name


def test_replace_lines_refuses_without_the_device_route():
    """a finder with a regex term has no device route: refused in HighlightLines' words before anything is uploaded"""
    from gofindthem_amd.finder import Finder, FinderError
    f = Finder.__new__(Finder)
    f._takes_device_route = lambda: False
    f._resident = lambda data: (_ for _ in ()).throw(AssertionError("uploaded"))
    with pytest.raises(FinderError) as ei:
        f.ReplaceLines(b"alice logged in\n")
    assert ei.value.code == _lib.GFT_E_UNSUPPORTED and "device route" in str(ei.value)
