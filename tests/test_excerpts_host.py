"""Excerpts on the host: gft_debug_excerpt_spans -- the kernels' passes walked tile by tile, carry trip by carry trip and lane by
lane through the header they compile -- against the reference of excerpts.py, written from the contract alone, on every fixed
case and the random batches; the cap protocol into guarded arrays, every output NULL on its own, and the refusals, which must
leave every output untouched.  All comparisons are exact; no device needed."""
import numpy as np
import pytest

import excerpts as X
from gofindthem_amd import _lib
from gofindthem_amd.engine import GftError, excerpt_shape, excerpt_spans_host
from gofindthem_amd.finder import Finder, FinderError, Match, PyRegexpEngine, SubstringEngine

TILE, TRIP = excerpt_shape() if hasattr(_lib.load(), "gft_debug_excerpt_shape") else (256, 1024)
GUARD = 3


def run(case, fill=0x00, **kw):
    blob, off, so, st, ln = case.arrays(fill)
    return excerpt_spans_host(blob, off, so, st, ln, case.before, case.after, case.runes, **kw)


def cut(r, guard=0):
    """the arrays of a result under exact caps, cut to their sizes; the guard entries must hold their pattern"""
    m, total = r["n_exc"], r["total"]
    sizes = {"out": total, "exc_off": m + 1, "exc_doc": m, "exc_start": m, "exc_span_off": m + 1}
    got = {"n_exc": m, "total": total}
    for k, v in r.items():
        if k in ("n_exc", "total"):
            continue
        if v is None:
            got[k] = np.zeros(0, dtype=np.uint64)
            continue
        n = sizes.get(k, v.size - guard)
        got[k] = v[:n]
        tail = v[n:]
        assert tail.size == guard and (tail.view(np.uint8) == 0xA5).all(), "%s: a store behind the cap" % k
    got["out"] = got["out"].tobytes()
    return got


def test_symbols_present():
    L = _lib.load()
    for name in ("gft_excerpt_spans_device", "gft_debug_excerpt_spans", "gft_debug_excerpt_shape", "gft_finder_excerpts_device"):
        assert hasattr(L, name) and name in _lib.SYMBOLS
    assert excerpt_shape() == (256, 1024)


def test_the_cases_tell_the_mutants_apart():
    assert X.assert_not_vacuous(TILE, TRIP)


@pytest.mark.parametrize("i", range(len(X.fixed_cases(TILE, TRIP))), ids=[c.name for c in X.fixed_cases(TILE, TRIP)])
def test_fixed_case(i):
    case = X.fixed_cases(TILE, TRIP)[i]
    for fill in (0x00, 0xBF):
        diff = X.same(cut(run(case, fill, guard=GUARD), GUARD), X.expected(case))
        assert diff is None, "%s, lead bytes %#x: %s" % (case.name, fill, diff)


def test_random_batches():
    for case in X.random_cases():
        diff = X.same(cut(run(case, 0xBF, guard=GUARD), GUARD), X.expected(case))
        assert diff is None, "%s: %s" % (case.name, diff)


def test_cap_protocol():
    case = X.fixed_cases(TILE, TRIP)[-2]                           # short excerpts round one of 5 004 bytes
    want = X.expected(case)
    m, total = want["n_exc"], want["total"]
    assert m >= 5 and total > 4096
    r = run(case, count_only=True)
    assert (r["n_exc"], r["total"]) == (m, total)
    # cap_exc one short: the entries below the cap, nothing at or past it; span_rel and doc_exc_off stay complete
    r = run(case, cap_exc=m - 1, cap_bytes=total, guard=GUARD)
    assert (r["n_exc"], r["total"]) == (m, total)
    assert r["exc_off"][:m].tolist() == want["exc_off"][:m] and r["exc_span_off"][:m].tolist() == want["exc_span_off"][:m]
    assert r["exc_doc"][:m - 1].tolist() == want["exc_doc"][:m - 1] and r["exc_start"][:m - 1].tolist() == want["exc_start"][:m - 1]
    for k, n in (("exc_off", m), ("exc_span_off", m), ("exc_doc", m - 1), ("exc_start", m - 1)):
        assert (r[k][n:].view(np.uint8) == 0xA5).all() and r[k][n:].size == GUARD, k
    assert r["span_rel"][:-GUARD].tolist() == want["span_rel"] and r["doc_exc_off"][:-GUARD].tolist() == want["doc_exc_off"]
    assert r["out"][:total].tobytes() == want["out"]
    # cap_bytes in the middle of the long excerpt
    capb = want["exc_off"][2] + 1000
    assert want["exc_off"][2] < capb < want["exc_off"][3]
    r = run(case, cap_exc=m, cap_bytes=capb, guard=GUARD)
    assert r["out"][:capb].tobytes() == want["out"][:capb] and (r["out"][capb:] == 0xA5).all() and r["out"][capb:].size == GUARD
    assert r["exc_off"][:m + 1].tolist() == want["exc_off"]


@pytest.mark.parametrize("name", ["out", "exc_off", "exc_doc", "exc_start", "exc_span_off", "span_rel", "doc_exc_off"])
def test_every_output_null_on_its_own(name):
    case = X.fixed_cases(TILE, TRIP)[-2]
    want = X.expected(case)
    r = run(case, omit=(name,), guard=GUARD)
    assert r[name] is None
    got = cut(r, GUARD)
    for k in X.ARRAYS:
        if k != name:
            assert got[k].tolist() == want[k], k
    if name != "out":
        assert got["out"] == want["out"]


def refused(case, **kw):
    blob, off, so, st, ln = case.arrays()
    out = None
    with pytest.raises(GftError) as ei:
        out = excerpt_spans_host(blob, off, so, st, ln, case.before, case.after, case.runes, **kw)
    assert ei.value.code == _lib.GFT_E_INVALID and out is None


def test_refusals_write_nothing():
    L = _lib.load()
    base = X.runs_case("ends that descend in the last tile", [TILE, 40])
    n = TILE + 40
    order, past = X.refusal_spans(base, n - 5)
    assert n - 5 >= TILE                                            # the pair that descends lies in the last tile
    for bad in (base.but("order", spans=[order]), base.but("past the end", spans=[past])):
        blob, off, so, st, ln = bad.arrays()
        # caps as the good batch would need them, every array guarded over its whole length
        good = run(base)
        m, total = good["n_exc"], good["total"]
        outs = {"out": np.full(total, 0xA5, np.uint8), "exc_off": np.full(m + 1, 0xA5A5A5A5A5A5A5A5, np.uint64),
                "exc_doc": np.full(m, 0xA5A5A5A5A5A5A5A5, np.uint64), "exc_start": np.full(m, 0xA5A5A5A5, np.uint32),
                "exc_span_off": np.full(m + 1, 0xA5A5A5A5A5A5A5A5, np.uint64), "span_rel": np.full(n, 0xA5A5A5A5, np.uint32),
                "doc_exc_off": np.full(2, 0xA5A5A5A5A5A5A5A5, np.uint64)}
        p = {k: v.ctypes.data for k, v in outs.items()}
        rc = L.gft_debug_excerpt_spans(blob.ctypes.data, off.ctypes.data, 1, so.ctypes.data, st.ctypes.data, ln.ctypes.data, 1, 1, 0, p["out"], total,
                                       p["exc_off"], p["exc_doc"], p["exc_start"], p["exc_span_off"], m, p["span_rel"], p["doc_exc_off"], None, None)
        assert rc == _lib.GFT_E_INVALID, bad.name
        for k, v in outs.items():
            assert (v.view(np.uint8) == 0xA5).all(), "%s: %s was written" % (bad.name, k)
    case = X.fixed_cases(TILE, TRIP)[0]
    blob, off, so, st, ln = case.arrays()
    with pytest.raises(GftError) as ei:
        excerpt_spans_host(blob, off, so, st, ln, 1, 1, flags=2)
    assert ei.value.code == _lib.GFT_E_INVALID
    with pytest.raises(GftError):
        excerpt_spans_host(blob, off[::-1].copy(), so, st, ln, 1, 1)
    with pytest.raises(GftError):
        excerpt_spans_host(blob, off, np.array([2, 0], np.uint64), st, ln, 1, 1)
    # overlapping buffers: span_rel over span_start, out inside the text
    m, total = C64(), C64()
    args = (blob.ctypes.data, off.ctypes.data, 1, so.ctypes.data, st.ctypes.data, ln.ctypes.data, 1, 1, 0)
    assert L.gft_debug_excerpt_spans(*args, None, 0, None, None, None, None, 0, st.ctypes.data, None, None, None) == _lib.GFT_E_INVALID
    assert L.gft_debug_excerpt_spans(*args, blob.ctypes.data + 4, 8, None, None, None, None, 0, None, None, None, None) == _lib.GFT_E_INVALID
    eo = np.zeros(8, np.uint64)
    assert L.gft_debug_excerpt_spans(*args, None, 0, eo.ctypes.data, eo.ctypes.data + 8, None, None, 2, None, None, None, None) == _lib.GFT_E_INVALID


def C64():
    import ctypes
    return ctypes.c_uint64(0)


def test_degenerate_batches():
    L = _lib.load()
    eo, eso, deo = (np.full(2, 7, np.uint64) for _ in range(3))
    assert L.gft_debug_excerpt_spans(None, None, 0, None, None, None, 3, 3, 1, None, 0, eo.ctypes.data, None, None, eso.ctypes.data, 0, None,
                                     deo.ctypes.data, None, None) == 0
    assert (eo[0], eso[0], deo[0]) == (0, 0, 0) and (eo[1], eso[1], deo[1]) == (7, 7, 7)
    # spans that begin behind span index 0: the arrays are indexed as the caller's
    case = X.fixed_cases(TILE, TRIP)[0]
    blob, off, so, st, ln = case.arrays()
    pad = 5
    r0 = excerpt_spans_host(blob, off, so, st, ln, 4, 4, False)
    r1 = excerpt_spans_host(blob, off, so + pad, np.concatenate([np.full(pad, 999, np.uint32), st]), np.concatenate([np.full(pad, 999, np.uint32), ln]),
                            4, 4, False)
    assert r1["out"].tobytes() == r0["out"].tobytes() and (r1["exc_span_off"] == r0["exc_span_off"] + pad).all()
    assert (r1["span_rel"][:pad].view(np.uint8) == 0xA5).all() and (r1["span_rel"][pad:] == r0["span_rel"]).all()


class NaiveEngine(SubstringEngine):
    """an injected substring engine: such a finder never takes the device route"""

    def BuildEngine(self, keywords, caseSensitive):
        self.keywords = list(keywords)

    def FindSubstrings(self, text):
        return [Match(text.find(k), k) for k in self.keywords if k in text]


def test_excerpt_lines_off_the_device_route_are_refused():
    """ExcerptLines has no host route -- the hit spans it cuts round have none --: a finder with an injected engine or with regex
    terms gets GFT_E_UNSUPPORTED, with or without a device, and before anything is uploaded"""
    for f, expr in ((Finder(NaiveEngine(), None, False, allow_no_device=True), '"ab"'),
                    (Finder(None, PyRegexpEngine(), True, allow_no_device=True), '"a" and r"b+"')):
        try:
            f.AddExpression(expr)
            assert f._takes_device_route() is False
            for source in (True, False):
                with pytest.raises(FinderError) as ei:
                    f.ExcerptLines(b"a bb ab\n", source=source)
                assert ei.value.code == _lib.GFT_E_UNSUPPORTED and "device route" in str(ei.value)
        finally:
            f.close()


def test_no_documents_never_reads_the_offsets():
    """n_docs == 0 with offset arrays given all the same: exc_span_off[0] is 0, as on the device, whatever span_off[0] holds"""
    L = _lib.load()
    nine = np.full(1, 9, np.uint64)
    eo, eso, deo = (np.full(2, 7, np.uint64) for _ in range(3))
    assert L.gft_debug_excerpt_spans(None, nine.ctypes.data, 0, nine.ctypes.data, None, None, 3, 3, 1, None, 0, eo.ctypes.data, None, None,
                                     eso.ctypes.data, 0, None, deo.ctypes.data, None, None) == 0
    assert (eo[0], eso[0], deo[0]) == (0, 0, 0) and (eo[1], eso[1], deo[1]) == (7, 7, 7)
