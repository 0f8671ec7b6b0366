"""Highlight on the host: gft_debug_mark_spans -- the runs by the excerpt's walk, the copy tile by tile and lane by lane through the
header the kernels compile -- against the reference of mark.py, written from the contract alone, on every fixed case, the span
counts round the walk's borders and the random batches; its runs against the excerpts of gft_debug_excerpt_spans(before = 0,
after = 0, flags = 0); the cap protocol into guarded arrays, every output NULL on its own, and the refusals, which must leave every
output untouched.  All comparisons are exact; no device needed."""
import ctypes as C

import numpy as np
import pytest

import mark as M
from gofindthem_amd import _lib
from gofindthem_amd.engine import GftError, excerpt_spans_host, mark_shape, mark_spans_host

TILE_SPANS, TRIP_TILES, CHUNK, TILE = mark_shape() if hasattr(_lib.load(), "gft_debug_mark_shape") else (256, 1024, 16, 4096)
GUARD = 3
NAMES = ("out", "out_off", "span_new", "doc_run_off")


def run(case, fill=0x00, **kw):
    blob, off, so, st, ln = case.arrays(fill)
    return mark_spans_host(blob, off, so, st, ln, case.open, case.close, **kw)


def cut(r, case, guard=0, cap=None):
    """the arrays of a result, cut to their sizes; the guard entries must hold their pattern"""
    total = r["total"] if cap is None else min(cap, r["total"])
    sizes = {"out": total, "out_off": len(case.docs) + 1, "span_new": sum(len(s) for s in case.spans), "doc_run_off": len(case.docs) + 1}
    got = {"n_runs": r["n_runs"], "total": r["total"]}
    for k in NAMES:
        v = r[k]
        if v is None:
            got[k] = [] if k != "out" else b""
            continue
        got[k] = v[:sizes[k]].tolist()
        tail = v[sizes[k]:]
        assert tail.size == guard and (tail.view(np.uint8) == 0xA5).all(), "%s: a store behind the cap" % k
    got["out"] = bytes(got["out"])
    return got


def test_symbols_present():
    L = _lib.load()
    for name in ("gft_mark_spans_device", "gft_debug_mark_spans", "gft_debug_mark_shape", "gft_finder_mark_device"):
        assert hasattr(L, name) and name in _lib.SYMBOLS
    assert mark_shape() == (256, 1024, 16, 4096) and (M.CHUNK, M.TILE, M.TRIP) == (16, 4096, 1024)
    header = open(_lib.__file__.replace("gofindthem_amd/_lib.py", "include/gft.h")).read()
    for name in ("gft_mark_spans_device", "gft_debug_mark_spans", "gft_debug_mark_shape", "gft_finder_mark_device", "GFT_MARK_MAX 255u"):
        assert name in header


def test_the_cases_tell_the_mutants_apart():
    assert M.assert_not_vacuous()


FIXED = M.fixed_cases()


@pytest.mark.parametrize("i", range(len(FIXED)), ids=[c.name for c in FIXED])
def test_fixed_case(i):
    case = FIXED[i]
    want = M.expected(case)
    for fill in (0x00, (case.open + case.close + b"<")[0]):
        for shift in (0, 1 + i % 15):
            assert M.same(cut(run(case, fill, guard=GUARD, shift=shift), case, GUARD), want), "%s, lead bytes %#x, out at +%d" % (case.name, fill, shift)


COUNTS = M.count_cases(TILE_SPANS, TRIP_TILES)


@pytest.mark.parametrize("i", range(len(COUNTS)), ids=[c.name for c in COUNTS])
def test_span_counts_round_the_walks_borders(i):
    case = COUNTS[i]
    assert M.same(cut(run(case, 0x3C, guard=GUARD, shift=9), case, GUARD), M.expected(case)), case.name


def test_random_batches():
    for seed in (1, 2, 3):
        for case in M.random_cases(seed):
            assert M.same(cut(run(case, 0xEE, guard=GUARD, shift=case.lead % 16), case, GUARD), M.expected(case)), case.name


def test_runs_are_the_excerpts_of_no_context():
    for case in FIXED + M.random_cases(4) + COUNTS[:3]:
        blob, off, so, st, ln = case.arrays()
        r = run(case)
        x = excerpt_spans_host(blob, off, so, st, ln, 0, 0, flags=0)
        m = x["n_exc"]
        assert r["n_runs"] == m and r["doc_run_off"].tolist() == x["doc_exc_off"].tolist(), case.name
        assert r["total"] == sum(len(d) for d in case.docs) + m * (len(case.open) + len(case.close)), case.name
        # every excerpt's bytes stand between an open and a close of the marked text, at the place its index arrays say
        out, ol, cl = bytes(r["out"][:r["total"]].tolist()) if r["out"] is not None else b"", len(case.open), len(case.close)
        exc = x["out"].tobytes() if x["out"] is not None else b""
        for k in range(m):
            d = int(x["exc_doc"][k])
            j = k - int(x["doc_exc_off"][d])
            at = int(r["out_off"][d]) + int(x["exc_start"][k]) + (j + 1) * ol + j * cl
            text = exc[int(x["exc_off"][k]):int(x["exc_off"][k + 1])]
            assert out[at - ol:at + len(text) + cl] == case.open + text + case.close, (case.name, k)


def test_cap_protocol():
    case = next(c for c in FIXED if c.name == "straddle_tile")
    want = M.expected(case)
    total = want["total"]
    assert run(case, count_only=True) == {"n_runs": want["n_runs"], "total": total}
    o = TILE - 2
    assert want["out"][o:o + 4] == b"<em>" and want["out"][o + 12:o + 17] == b"</em>"
    for cb in (0, 1, 100, o + 2, o + 14, 96, 107, TILE, o + 4, total - 1, total, total + 5):
        for shift in (0, 5):
            r = run(case, 0x3C, cap_bytes=cb, guard=GUARD, shift=shift)
            if cb > total:                                          # (room to spare stays as it was)
                assert (r["out"][total:] == 0xA5).all()
                r["out"] = r["out"][:total + GUARD]
            got = cut(r, case, GUARD, cb)
            assert got["out"] == want["out"][:cb] and all(got[k] == want[k] for k in M.ARRAYS), cb
            assert (got["n_runs"], got["total"]) == (want["n_runs"], total)


@pytest.mark.parametrize("name", NAMES)
def test_every_output_null_on_its_own(name):
    for case in (next(c for c in FIXED if c.name == "touch_across_docs"), next(c for c in FIXED if c.name == "empty_docs")):
        want = M.expected(case)
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
    past = spans1[:-1] + [(spans1[-1][0], len(base.docs[1]))]
    total = M.expected(base)["total"]

    def refused(case, what, **kw):
        blob, off, so, st, ln = case.arrays()
        kw.setdefault("open", case.open)
        kw.setdefault("close", case.close)
        outs = [np.full(total, 0xA5, np.uint8), np.full(len(case.docs) + 1, 0xA5A5A5A5A5A5A5A5, np.uint64), np.full(st.size, 0xA5A5A5A5, np.uint32),
                np.full(len(case.docs) + 1, 0xA5A5A5A5A5A5A5A5, np.uint64)]
        n_runs, n_bytes = C.c_uint64(77), C.c_uint64(77)
        flags = kw.pop("flags", 0)
        o, c = kw["open"], kw["close"]
        rc = L.gft_debug_mark_spans(blob.ctypes.data, kw.get("off", off).ctypes.data, len(case.docs), kw.get("so", so).ctypes.data, st.ctypes.data,
                                    ln.ctypes.data, o, kw.get("open_len", len(o or b"")), c, kw.get("close_len", len(c or b"")), flags,
                                    outs[0].ctypes.data, total, outs[1].ctypes.data, outs[2].ctypes.data, outs[3].ctypes.data,
                                    C.byref(n_runs), C.byref(n_bytes))
        assert rc == _lib.GFT_E_INVALID, what
        assert (n_runs.value, n_bytes.value) == (0, 0), what
        for a in outs:
            assert (a.view(np.uint8) == 0xA5).all(), what

    refused(base.but("order", spans=[base.spans[0], order]), "ends that descend")
    refused(base.but("past", spans=[base.spans[0], past]), "a span past its document")
    refused(base, "flags", flags=1)
    refused(base, "a long open", open=b"x" * 256)
    refused(base, "a long close", close=b"y" * 256)
    refused(base, "a NULL open with a length", open=None, open_len=2)
    refused(base, "a NULL close with a length", close=None, close_len=2)
    _, off, so, _, _ = base.arrays()
    bad_off = off.copy()
    bad_off[1] = bad_off[2] + 1
    refused(base, "document offsets that descend", off=bad_off)
    bad_so = so.copy()
    bad_so[1] = bad_so[2] + 1
    refused(base, "span offsets that descend", so=bad_so)
    # a document that would reach 4 GiB once marked: found from the offsets alone, no text is read
    one = M.Case("big", [b"abc"], [[(1, 1)]])
    refused(one, "a document that reaches 4 GiB once marked", off=np.array([0, (1 << 32) - 8], np.uint64))
    refused(one, "a document of 4 GiB", off=np.array([0, 1 << 32], np.uint64))
    # an output that is an input
    blob, off, so, st, ln = base.arrays()
    st = st.copy()
    rc = L.gft_debug_mark_spans(blob.ctypes.data, off.ctypes.data, 2, so.ctypes.data, st.ctypes.data, ln.ctypes.data, b"<", 1, b">", 1, 0, None, 0, None,
                                st.ctypes.data, None, None, None)
    assert rc == _lib.GFT_E_INVALID and st.tolist() == base.arrays()[3].tolist()
    with pytest.raises(GftError):
        run(base, flags=2)
    # no documents: the offsets are not read; the two offset arrays get their 0
    oo, ro = np.full(2, 7, np.uint64), np.full(2, 7, np.uint64)
    assert L.gft_debug_mark_spans(None, None, 0, None, None, None, b"<", 1, b">", 1, 0, None, 0, oo.ctypes.data, None, ro.ctypes.data, None, None) == 0
    assert oo.tolist() == [0, 7] and ro.tolist() == [0, 7]
