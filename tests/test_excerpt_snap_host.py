"""Excerpts snapped to word or line borders, on the host: the two edge walks of csrc/gft_excerpt_piece.hpp alone
(gft_debug_excerpt_snap_edges) at every position of every fixed document against the reference of snap_cases.py; the properties
the excerpt pipeline needs of a window -- monotone, contained, bounded by the reach -- at every edge of 3 000 random documents;
the host twin gft_debug_excerpt_spans_snap on every case with every output array compared; no snap bit = gft_debug_excerpt_spans
byte for byte; the refusals; tools/excerpt_snap_check.cpp built with the address and undefined-behaviour sanitizers and run.  All
comparisons are exact; no device needed."""
import ctypes as C
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import excerpts as X
import snap_cases as S
import word_cases as W
from gofindthem_amd import _lib
from gofindthem_amd.engine import Engine, GftError, excerpt_shape, excerpt_snap_edges, excerpt_spans_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = excerpt_shape()[0]
FIXED = S.fixed_cases(TILE)
GUARD = 3
REACHES = (0, 1, 2, 3, 5, 100)


def run(case, fill=0x00, span_lead=0, span_tail=0, **kw):
    blob, off, so, st, ln = case.arrays(fill, span_lead, span_tail)
    return excerpt_spans_host(blob, off, so, st, ln, case.before, case.after, flags=case.flags, reach=case.reach, snap_call=True, **kw)


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
        assert v[n:].size == guard and (v[n:].view(np.uint8) == 0xA5).all(), "%s: a store behind the cap" % k
    got["out"] = got["out"].tobytes()
    return got


def test_symbols_exported_and_declared():
    L = _lib.load()
    for name in ("gft_excerpt_spans_snap_device", "gft_debug_excerpt_spans_snap", "gft_debug_excerpt_snap_edges", "gft_finder_excerpts_snap_device"):
        assert hasattr(L, name) and name in _lib.SYMBOLS, name
    header = open(os.path.join(ROOT, "include", "gft.h")).read()
    for text in ("#define GFT_EXCERPT_WORDS 2u", "#define GFT_EXCERPT_LINES 4u", "#define GFT_EXCERPT_REACH_MAX 4096u"):
        assert text in header, text


def test_the_cases_tell_the_mutants_apart():
    assert set(S.assert_not_vacuous(TILE)) == set(S.MUTANTS)


def fixed_documents():
    """(document, flags, reach) of the fixed cases, each once"""
    seen = {}
    for c in FIXED:
        for d in c.docs:
            seen.setdefault((d, c.flags, c.reach), None)
    return list(seen)


def c_edges(doc, flags, reach):
    """gft_debug_excerpt_snap_edges(doc, p, p) for every p -> (starts, ends)"""
    L = _lib.load()
    a = np.frombuffer(doc, dtype=np.uint8)
    ptr = a.ctypes.data if a.size else None
    lo, hi = C.c_uint64(0), C.c_uint64(0)
    starts, ends = [], []
    for p in range(len(doc) + 1):
        assert L.gft_debug_excerpt_snap_edges(ptr, len(doc), p, p, flags, reach, C.byref(lo), C.byref(hi)) == 0
        starts.append(lo.value)
        ends.append(hi.value)
    return starts, ends


def test_the_linear_reference_is_the_walk():
    """snap_cases.all_edges, which the sweeps below use, against the walks themselves: every position of every fixed document of up
    to 600 bytes, at the case's reach and at the sweep's"""
    n = 0
    for doc, flags, reach in fixed_documents():
        if len(doc) > 600:
            continue
        for r in {reach} | set(REACHES):
            starts, ends = S.all_edges(doc, flags, r)
            for p in range(len(doc) + 1):
                assert (starts[p], ends[p]) == S.snap_edges(doc, p, p, flags, r), (doc, flags, r, p)
            n += 1
    assert n > 500


def test_edges_at_every_position_of_every_fixed_document():
    docs = fixed_documents()
    assert any(len(d) > S.REACH_MAX for d, _, _ in docs) and any(f & S.WORDS for _, f, _ in docs) and any(f & S.LINES for _, f, _ in docs)
    for doc, flags, reach in docs:
        assert c_edges(doc, flags, reach) == S.all_edges(doc, flags, reach), (doc[:40], flags, reach)
    # a window with two different edges: the two walks do not know of each other
    doc = b"one two\nthree four"
    for flags in (S.WORDS, S.LINES, S.LINES | S.RUNES):
        for lo in range(len(doc) + 1):
            for hi in range(lo, len(doc) + 1):
                assert excerpt_snap_edges(doc, lo, hi, None, 4, flags=flags) == S.snap_edges(doc, lo, hi, flags, 4)


def test_edge_walks_are_monotone_contained_and_bounded():
    """what the excerpt's passes need of a window, at every edge of 3 000 random documents over word_cases.SYMBOLS: the snapped edge
    is monotone in the edge it starts from, stays inside [0, L], only grows the window and moves at most `reach` bytes from the
    rune-snapped edge.  Checked on the reference and, position by position, on the library against it"""
    rng = random.Random(20261021)
    for i in range(3000):
        doc = b"".join(rng.choice(W.SYMBOLS) for _ in range(rng.randint(0, 24)))
        L = len(doc)
        for flags in (S.WORDS, S.LINES):
            snapped = [S.rune_snap(doc, p, p) if flags & S.WORDS else (p, p) for p in range(L + 1)]
            for reach in REACHES:
                starts, ends = S.all_edges(doc, flags, reach)
                if i % 3 == 0:
                    assert c_edges(doc, flags, reach) == (starts, ends), (doc, flags, reach)
                for p in range(L + 1):
                    lo, hi = snapped[p]
                    assert 0 <= starts[p] <= lo <= p <= hi <= ends[p] <= L, (doc, flags, reach, p)
                    assert lo - starts[p] <= reach and ends[p] - hi <= reach, (doc, flags, reach, p)
                    assert p == 0 or (starts[p - 1] <= starts[p] and ends[p - 1] <= ends[p]), (doc, flags, reach, p)
                if reach == 0:
                    assert [(s, e) for s, e in zip(starts, ends)] == snapped
    # ... and the word snap WITHOUT the implied rune snap is not monotone: that is why the bit implies it
    doc = "a中b".encode()
    ends = [S.snap_edges(doc, p, p, S.WORDS, 64, "no_implied_runes")[1] for p in range(len(doc) + 1)]
    assert ends != sorted(ends)


@pytest.mark.parametrize("i", range(len(FIXED)), ids=[c.name for c in FIXED])
def test_fixed_case(i):
    case = FIXED[i]
    want = S.expected(case)
    for fill in (0x00, 0xBF, ord("a")):
        diff = X.same(cut(run(case, fill, guard=GUARD), GUARD), want)
        assert diff is None, "%s, lead bytes %#x: %s" % (case.name, fill, diff)


def test_fixed_cases_behind_a_span_base():
    for case in S.small(FIXED)[::3]:
        got = cut(run(case, ord("a"), 3, 2, guard=GUARD), GUARD)
        diff = X.same(got, S.expected(case, None, 3, 2), untouched=0xA5A5A5A5)
        assert diff is None, "%s: %s" % (case.name, diff)


def test_random_batches():
    for case in S.random_cases():
        diff = X.same(cut(run(case, ord("a"), guard=GUARD), GUARD), S.expected(case))
        assert diff is None, "%s: %s" % (case.name, diff)


def test_words_without_runes_is_words_with_runes():
    a = next(c for c in FIXED if c.name == "words, runes not given")
    b = next(c for c in FIXED if c.name == "words, runes given")
    assert a.flags == S.WORDS and b.flags == S.WORDS | S.RUNES and S.expected(a) == S.expected(b)
    assert X.same(cut(run(a)), cut(run(b))) is None
    assert S.expected(a) != S.expected(a, "no_implied_runes")


def test_no_snap_bit_is_the_plain_call_byte_for_byte():
    T, K = excerpt_shape()
    cases = [c for c in X.fixed_cases(T, K) if sum(map(len, c.spans)) < 5000] + list(X.random_cases())[:20]
    for case in cases:
        blob, off, so, st, ln = case.arrays(0xBF)
        plain = excerpt_spans_host(blob, off, so, st, ln, case.before, case.after, case.runes, guard=GUARD)
        for reach in (0, 64, S.REACH_MAX):
            snapped = excerpt_spans_host(blob, off, so, st, ln, case.before, case.after, case.runes, guard=GUARD, reach=reach, snap_call=True)
            for k in plain:
                assert (plain[k] is None and snapped[k] is None) or np.array_equal(plain[k], snapped[k]), (case.name, reach, k)
    # reach 0 with a snap bit: the plain call with the rune snap (words) or as given (lines)
    for case in S.small(FIXED):
        blob, off, so, st, ln = case.arrays(ord("a"))
        plain = excerpt_spans_host(blob, off, so, st, ln, case.before, case.after, case.runes or case.snap == "words")
        snapped = excerpt_spans_host(blob, off, so, st, ln, case.before, case.after, flags=case.flags, reach=0, snap_call=True)
        for k in plain:
            assert (plain[k] is None and snapped[k] is None) or np.array_equal(plain[k], snapped[k]), (case.name, k)


def test_cap_protocol():
    case = next(c for c in FIXED if c.name == "exactly the hit lines, adjacent lines apart")
    want = S.expected(case)
    m, total = want["n_exc"], want["total"]
    assert m >= 4
    r = run(case, count_only=True)
    assert (r["n_exc"], r["total"]) == (m, total)
    r = run(case, cap_exc=m - 1, cap_bytes=total - 5, guard=GUARD)
    assert (r["n_exc"], r["total"]) == (m, total)
    assert r["exc_off"][:m].tolist() == want["exc_off"][:m] and r["exc_doc"][:m - 1].tolist() == want["exc_doc"][:m - 1]
    assert r["out"][:total - 5].tobytes() == want["out"][:total - 5]
    for k, n in (("exc_off", m), ("exc_span_off", m), ("exc_doc", m - 1), ("exc_start", m - 1), ("out", total - 5)):
        assert (r[k][n:].view(np.uint8) == 0xA5).all() and r[k][n:].size == GUARD, k


def test_refusals():
    L = _lib.load()
    case = FIXED[0]
    blob, off, so, st, ln = case.arrays()
    for flags, reach in ((S.WORDS | S.LINES, 1), (S.WORDS | S.LINES | S.RUNES, 0), (8, 1), (0x80000002, 1), (S.WORDS, S.REACH_MAX + 1),
                         (S.LINES, 0xFFFFFFFF), (0, S.REACH_MAX + 1)):
        with pytest.raises(GftError) as ei:
            excerpt_spans_host(blob, off, so, st, ln, 1, 1, flags=flags, reach=reach, snap_call=True)
        assert ei.value.code == _lib.GFT_E_INVALID, (flags, reach)
        with pytest.raises(GftError) as ei:
            excerpt_snap_edges(b"ab cd", 1, 2, None, reach, flags=flags)
        assert ei.value.code == _lib.GFT_E_INVALID, (flags, reach)
    excerpt_spans_host(blob, off, so, st, ln, 1, 1, flags=S.WORDS, reach=S.REACH_MAX, snap_call=True)
    # the plain calls still know one flag alone
    for flags in (S.WORDS, S.LINES, S.WORDS | S.RUNES):
        with pytest.raises(GftError) as ei:
            excerpt_spans_host(blob, off, so, st, ln, 1, 1, flags=flags)
        assert ei.value.code == _lib.GFT_E_INVALID
    # the edges call: a window that is none
    lo, hi = C.c_uint64(7), C.c_uint64(7)
    a = np.frombuffer(b"ab cd", dtype=np.uint8)
    for w in ((3, 2), (0, 6), (6, 6)):
        assert L.gft_debug_excerpt_snap_edges(a.ctypes.data, 5, w[0], w[1], S.WORDS, 4, C.byref(lo), C.byref(hi)) == _lib.GFT_E_INVALID
    assert (lo.value, hi.value) == (7, 7)
    # a refused batch writes nothing, as in the plain call
    bad = case.but("past the end", spans=[[(len(d), 1)] for d in case.docs])
    with pytest.raises(GftError):
        run(bad)
    with pytest.raises(ValueError):
        Engine.excerpt_spans_host(blob, off, so, st, ln, snap="sentences")


def test_engine_wrapper():
    case = next(c for c in FIXED if c.name == "exactly the hit lines, adjacent lines apart")
    blob, off, so, st, ln = case.arrays()
    out, exc_off, exc_doc, exc_start, exc_span_off, span_rel, doc_exc_off = Engine.excerpt_spans_host(blob, off, so, st, ln, 0, 0, False, snap="lines",
                                                                                                        reach=S.REACH_MAX)
    pieces = [out[a:b].tobytes() for a, b in zip(exc_off, exc_off[1:])]
    assert pieces == [b"09:01 ERROR disk full", b"09:03 ERROR again", b"09:04 ERROR thrice", b"09:03 ERROR again", b"09:04 ERROR thrice"]
    assert exc_doc.tolist() == [0, 0, 0, 2, 2] and doc_exc_off.tolist() == [0, 3, 3, 5]
    words = Engine.excerpt_spans_host(b"failed to authenticate user admin", [0, 33], [0, 1], [10, ], [12], 3, 3, snap="words")
    assert words[0].tobytes() == b"to authenticate user" and words[3].tolist() == [7]
    plain = Engine.excerpt_spans_host(b"failed to authenticate user admin", [0, 33], [0, 1], [10, ], [12], 3, 3)
    assert plain[0].tobytes() == b"to authenticate us"


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_excerpt_snap_check_under_sanitizers(tmp_path):
    exe = str(tmp_path / "excerpt_snap_check")
    csrc = os.path.join(ROOT, "gofindthem_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", ROOT,
           os.path.join(ROOT, "tools", "excerpt_snap_check.cpp"), os.path.join(csrc, "excerpt_host.cpp"), os.path.join(csrc, "words_host.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, cwd=ROOT)
    r = subprocess.run([exe, "120"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
