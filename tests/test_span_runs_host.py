"""The four host walks that take "the spans [span_off[0], span_off[n_docs]) of the caller's span arrays" -- gft_debug_excerpt_spans,
gft_debug_mark_spans, gft_debug_redact_spans, gft_debug_map_spans_to_source -- with span_off[0] != 0: the fixed cases of the four
case modules handed over behind 1, T - 1, T and T + 1 entries of poison (T the walk's tile), the random batches cut at random
[a, b), partitions into 1, 2, 3 and n_docs runs that write into the same parallel arrays, the refusals and the overlap checks under
a base.  restrict() of the reference's answer for the whole batch is first proven equal, on the CPU alone, to the reference's answer
for the run built as a case of its own.  All comparisons are exact; no device needed."""
import ctypes as C

import numpy as np
import pytest

import excerpts as X
import lowermap_cases as LM
import mark as M
import span_runs as R
import spans as S
import tolower_cases as TC
from gofindthem_amd import _lib
from gofindthem_amd.engine import excerpt_shape, lowermap_shape, mark_shape, spans_shape

L = _lib.load()
XT, XTRIP = excerpt_shape()
MT = mark_shape()[0]
FT = spans_shape()[1]
LT = lowermap_shape()[3]
TAIL = 2


def bases(tile):
    return (1, tile - 1, tile, tile + 1)


@pytest.fixture(scope="module")
def drv():
    calls = {"excerpt": L.gft_debug_excerpt_spans, "mark": L.gft_debug_mark_spans, "redact": L.gft_debug_redact_spans,
             "map": L.gft_debug_map_spans_to_source}
    return R.Driver(R.HostMem(), calls, X, M, S, LM, _lib.GFT_E_INVALID)


def test_the_tiles_are_the_walks_own():
    assert (XT, MT, FT, LT) == (256, 256, 64, 64)


def test_the_cases_tell_the_base_mutants_apart():
    """each module's assert_not_vacuous names the fixed cases that catch every wrong reading of the base"""
    told = X.assert_not_vacuous(XT, XTRIP)
    assert set(X.BASE_MUTANTS) <= set(told) and "windows touch in the blob" in told["first_from_k"]
    told = M.assert_not_vacuous()
    assert set(M.BASE_MUTANTS) <= set(told) and "touch_across_docs" in told["first_from_k"]
    assert S.assert_fill_not_vacuous()
    told = LM.assert_not_vacuous()
    assert all(told[m] for m in LM.BASE_MUTANTS)


# ---- the cases -----------------------------------------------------------------------------------------------------------------
def excerpt_cases():
    """the fixed cases that cross a tile border, put a document border on one, have documents without spans in front, in the middle
    and at the end, empty documents, one document, no spans at all; and the one whose documents' windows touch in the blob"""
    names = ("gap 0", "the whole document", "a document of no bytes", "documents without spans between", "windows touch in the blob", "no spans at all",
             "a run ends at a tile border", "a run crosses a tile border", "a document border on a tile border", "a later span reaches further back",
             "a lead byte is not the document's", "doc_off[0] != 0")
    by = {c.name: c for c in X.fixed_cases(XT, XTRIP)}
    cases = [by[n] for n in names]
    c = by["documents without spans between"]
    cases.append(c.but("documents without spans at the end", docs=c.docs + [b"tail", b""], spans=c.spans + [[], []]))
    return cases


def mark_cases():
    names = ("run_first_byte", "empty_run_at_ends", "empty_docs", "docs_without_spans", "touch_across_docs", "second_doc_ranks", "no_spans",
             "text_residue_5", "straddle_tile", "many_insertions_in_tile")
    by = {c.name: c for c in M.fixed_cases()}
    c = by["docs_without_spans"]
    return [by[n] for n in names] + M.count_cases(MT, 1024)[:3] + [
        c.but("docs_without_spans_at_both_ends", docs=[b"", c.docs[0]] + c.docs + [c.docs[0], b""], spans=[[], []] + c.spans + [[], []])]


def map_batches():
    docs, spans = LM.base_docs()
    d130 = [("É%d İ" % i).encode() for i in range(130)]                # more than two tiles of spans, a document each
    return {"base": (docs, spans), "130 documents": (d130, [(np.array([i % 3]), np.array([2])) for i in range(130)]),
            "one document": (docs[:1], spans[:1]), "no spans": (docs, [(np.zeros(0, np.int64),) * 2] * len(docs))}


XC, MC = excerpt_cases(), mark_cases()


@pytest.mark.parametrize("i", range(len(XC)), ids=[c.name for c in XC])
def test_excerpt_fixed_cases_behind_a_base(drv, i):
    for s0 in bases(XT):
        drv.excerpt_case(XC[i], s0, TAIL, fill=0xBF if s0 & 1 else 0x00)


@pytest.mark.parametrize("i", range(len(MC)), ids=[c.name for c in MC])
def test_mark_fixed_cases_behind_a_base(drv, i):
    for s0 in bases(MT):
        drv.mark_case(MC[i], s0, TAIL, fill=0x3C if s0 & 1 else 0x00, shift=s0 % 16)


@pytest.mark.parametrize("s0", bases(FT))
def test_fill_cases_behind_a_base(drv, s0):
    """every fill case, the refused ones too: the poison at s0 - 1 and s0 + n is not what refuses them"""
    for f in S.fill_cases(s0, TAIL):
        drv.fill_case(f)


@pytest.mark.parametrize("name", sorted(map_batches()))
def test_map_batches_behind_a_base(drv, name):
    docs, spans = map_batches()[name]
    for s0 in bases(LT):
        for doc_lead in (0, 5):
            drv.map_case(docs, spans, s0, TAIL, doc_lead, what=name)


# ---- restrict() against the run as a case of its own: two routes, no library --------------------------------------------------
def random_cuts(n_docs, rng, k=2):
    out = []
    for _ in range(k):
        a = int(rng.integers(0, n_docs))
        out.append((a, int(rng.integers(a + 1, n_docs + 1))))
    return out


def test_restrict_is_the_reference_of_the_run_as_its_own_case():
    rng = np.random.default_rng(7)
    for case in X.random_cases() + tuple(XC):
        arrays, want = case.arrays(), X.expected(case)
        for a, b in random_cuts(len(case.docs), rng):
            own, lead, tail = R.own_excerpt(case, arrays[2], arrays[3].size, a, b, arrays[1])
            d = R.differs(R.restrict(R.Whole("excerpt", arrays, want), a, b), X.expected(own, None, lead, tail))
            assert d is None, "%s [%d, %d): %s" % (case.name, a, b, d)
            assert np.array_equal(R.cut(arrays, a, b)[2], own.arrays(0, lead, tail)[2]) and np.array_equal(R.cut(arrays, a, b)[1], own.arrays()[1])
    for case in M.random_cases(5) + MC:
        if not case.docs:
            continue
        arrays, want = case.arrays(), M.expected(case)
        for a, b in random_cuts(len(case.docs), rng):
            own, lead, tail = R.own_mark(case, arrays[2], arrays[3].size, a, b, arrays[1])
            d = R.differs(R.restrict(R.Whole("mark", arrays, want), a, b), M.expected(own, None, lead, tail))
            assert d is None, "%s [%d, %d): %s" % (case.name, a, b, d)
    for f in S.fill_cases():
        if not f.ok:
            continue
        arrays = (f.blob, f.doc_off, f.span_off, f.start, f.length)
        for a, b in random_cuts(len(f.doc_off) - 1, rng):
            own = R.own_fill(S, f, a, b)
            assert R.restrict(R.Whole("redact", arrays, S.redact_reference(f)), a, b) == S.redact_reference(own), (f.name, a, b)
    docs, spans = LM.base_docs()
    so, st, ln = LM.flat(spans)
    whole = LM.expected(docs, spans)
    for a, b in random_cuts(len(docs), rng, 6):
        own = LM.expected(docs[a:b], spans[a:b], int(so[a]), st.size - int(so[b]))
        got = R.restrict(R.Whole("map", (None, None, so, st, ln), whole[1:]), a, b)
        # (outside the run the cut holds the other documents' lowered spans, the own case poison: compare inside, and the borders)
        lo, hi = int(so[a]), int(so[b])
        assert np.array_equal(got[0][lo:hi], own[1][lo:hi]) and np.array_equal(got[1][lo:hi], own[2][lo:hi]), (a, b)
        assert np.array_equal(got[0][:lo], st[:lo]) and np.array_equal(got[0][hi:], st[hi:]) and (own[1][:lo] == R.FULL).all()


# ---- random batches cut at random [a, b) ----------------------------------------------------------------------------------------
def test_excerpt_random_batches_cut(drv):
    rng = np.random.default_rng(11)
    for case in X.random_cases():
        want = X.expected(case)
        for a, b in random_cuts(len(case.docs), rng):
            drv.excerpt_cut(case, a, b, want, at=a % 3)


def test_mark_random_batches_cut(drv):
    rng = np.random.default_rng(12)
    for case in M.random_cases(6):
        if case.docs:
            want = M.expected(case)
            for a, b in random_cuts(len(case.docs), rng):
                drv.mark_cut(case, a, b, want)
    for case in M.count_cases(MT, 1024)[:3]:                         # the second document alone: a base of about half a tile
        drv.mark_cut(case, 1, 2, M.expected(case))


def test_fill_random_batches_cut(drv):
    rng = np.random.default_rng(13)
    for f in S.fill_cases():
        if f.ok:
            want = S.redact_reference(f)
            for a, b in random_cuts(len(f.doc_off) - 1, rng, 3):
                drv.fill_cut(f, a, b, want)


def test_map_random_batches_cut(drv):
    rng = np.random.default_rng(14)
    docs = TC.random_docs()[:400]
    spans = [LM.every_byte(d, n_random=3, seed=i) if i % 5 else (np.zeros(0, np.int64),) * 2 for i, d in enumerate(docs)]
    for a, b in random_cuts(len(docs), rng, 6) + [(0, 1), (399, 400)]:
        drv.map_case(docs, spans, 0, 0, doc_lead=3, a=a, b=b, what="random documents")


# ---- partitions: the runs write into the same parallel arrays ----------------------------------------------------------------
def parts_of(n_docs):
    return sorted({p for p in (1, 2, 3, n_docs) if p <= n_docs})


def test_excerpt_partitions(drv):
    rng = np.random.default_rng(21)
    for case in list(X.random_cases()[:12]) + [X.random_cases()[-1]] + XC:
        if len(case.docs) > 100:
            continue
        want = X.expected(case, None, 3, TAIL)
        for p in parts_of(len(case.docs)):
            drv.excerpt_partition(case, R.partition(len(case.docs), p, rng), want, 3, TAIL)


def test_mark_partitions(drv):
    rng = np.random.default_rng(22)
    for case in M.random_cases(7)[:15] + MC:
        if not case.docs:
            continue
        want = M.expected(case, None, 3, TAIL)
        for p in parts_of(len(case.docs)):
            drv.mark_partition(case, R.partition(len(case.docs), p, rng), want, 3, TAIL)


def test_fill_and_map_partitions(drv):
    rng = np.random.default_rng(23)
    for f in S.fill_cases(5, TAIL):
        n = len(f.doc_off) - 1
        if f.ok:
            for p in parts_of(n) if n < 300 else (1, 2, 3):
                drv.fill_partition(f, R.partition(n, p, rng))
    for name, (docs, spans) in map_batches().items():
        for p in parts_of(len(docs)):
            drv.map_partition(docs, spans, R.partition(len(docs), p, rng), 5, TAIL, doc_lead=2)


# ---- refusals under a base -------------------------------------------------------------------------------------------------------
def test_excerpt_and_mark_refusals_under_a_base(drv):
    """a span past its document at index s0 and at s0 + n - 1; ends that descend between s0 and s0 + 1; span_off[n_docs] <
    span_off[0]: each refused with every output untouched"""
    body = X._rand_bytes(60, 3)
    good = [[(2, 3), (10, 2), (30, 5)], [(1, 1), (20, 4)]]
    first_past = [[(58, 3), (59, 1), (59, 1)], good[1]]            # index s0: start + len = 61 > 60, the ends still ascending
    last_past = [good[0], [(1, 1), (57, 4)]]                       # index s0 + n - 1
    descend = [[(2, 9), (3, 2), (30, 5)], good[1]]                 # end 11 at s0, end 5 at s0 + 1
    for s0 in (1, XT):
        for what, spans in (("past at s0", first_past), ("past at s0 + n - 1", last_past), ("ends descend at s0", descend)):
            drv.excerpt_refused(X.Case(what, [body, body], spans, 2, 2), s0, TAIL, what=what)
            drv.mark_refused(M.Case(what, [body, body], spans), s0, TAIL, what=what)
        ok = X.Case("good", [body, body], good, 2, 2)
        drv.excerpt_case(ok, s0, TAIL)                              # (the same batch with nothing wrong is taken)
        drv.excerpt_refused(ok, s0, TAIL, so=[s0 + 5, s0 + 3, s0], what="span_off[n_docs] < span_off[0]")
        drv.excerpt_refused(ok, s0, TAIL, so=[s0, s0 + 4, s0 + 3], what="span offsets descend")
        okm = M.Case("good", [body, body], good)
        drv.mark_case(okm, s0, TAIL)
        drv.mark_refused(okm, s0, TAIL, so=[s0 + 5, s0 + 3, s0], what="span_off[n_docs] < span_off[0]")
        drv.mark_refused(okm, s0, TAIL, so=[s0, s0 + 4, s0 + 3], what="span offsets descend")


def test_fill_and_map_refusals_under_a_base(drv):
    for s0 in (1, FT):
        for spans, what in (([[(38, 3), (0, 1)], [(5, 5)]], "past at s0"), ([[(0, 4)], [(5, 5), (36, 5)]], "past at s0 + n - 1")):
            drv.fill_refused(S.fill_case(what, [40, 40], spans, seed=3, lead=2, span_lead=s0, span_tail=TAIL), what)
        f = S.fill_case("good", [40, 40], [[(0, 4)], [(5, 5)]], seed=4, span_lead=s0, span_tail=TAIL)
        drv.fill_case(f)
        drv.fill_refused(f._replace(span_off=np.array([s0 + 2, s0 + 1, s0], np.uint64)), "span_off[n_docs] < span_off[0]")
    docs = ["CAFÉ İ one".encode(), "İİ two Ⱥ".encode()]
    Bs = [LM.lowered_len(d) for d in docs]
    for s0 in (1, LT):
        for bad, what in (([(np.array([Bs[0] - 1, 1]), np.array([2, 1])), (np.array([0]), np.array([1]))], "past at s0"),
                          ([(np.array([0]), np.array([1])), (np.array([1, Bs[1]]), np.array([1, 1]))], "past at s0 + n - 1")):
            assert LM.expected(docs, bad, s0, TAIL) is None
            drv.map_refused(docs, *LM.flat(bad, s0, TAIL), what=what)
        good = [(np.array([0, 2]), np.array([3, 1]))] * 2
        so, st, ln = LM.flat(good, s0, TAIL)
        drv.map_refused(docs, [s0 + 4, s0 + 2, s0], st, ln, what="span_off[n_docs] < span_off[0]")
        drv.map_case(docs, good, s0, TAIL, what="good")


# ---- the overlap checks cover [s0, s0 + n) of each array, no more ----------------------------------------------------------------
def test_overlap_checks_under_a_base():
    """an output that overlaps only entries below s0 of a span array is no overlap; one that overlaps one entry inside is"""
    s0, n_out = 40, 8
    body = X._rand_bytes(60, 5)
    case = X.Case("overlap", [body, body], [[(2, 3), (10, 2)], [(1, 1), (20, 4)]], 2, 2, runes=False)
    blob, off, so, st, ln = case.arrays(0, s0, TAIL)
    want = X.expected(case, None, s0, TAIL)
    m, total = want["n_exc"], want["total"]
    assert m + 1 <= n_out and s0 >= 2 * n_out + 2
    head = (blob.ctypes.data, off.ctypes.data, 2, so.ctypes.data, st.ctypes.data, ln.ctypes.data)
    mwant = M.expected(M.Case("overlap", case.docs, case.spans, b"<", b">"), None, s0, TAIL)
    for arr, what in ((st, "span_start"), (ln, "span_len")):
        # exc_off / out_off as 8-byte entries that end `gap` bytes below entry s0 of the 4-byte array: gap 0 touches nothing inside
        for gap, rc_want in ((0, 0), (-4, _lib.GFT_E_INVALID)):
            keep = arr.copy()
            at = arr.ctypes.data + 4 * s0 - 8 * (m + 1) - gap
            rc = L.gft_debug_excerpt_spans(*head, 2, 2, 0, None, 0, at, None, None, None, m, None, None, None, None)
            assert rc == rc_want, "excerpt: exc_off ending %d bytes below %s[s0]" % (gap, what)
            if rc == 0:
                got = np.frombuffer(C.string_at(at, 8 * (m + 1)), np.uint64).tolist()
                assert got == want["exc_off"] and np.array_equal(arr[s0:], keep[s0:])
            else:
                assert np.array_equal(arr, keep), "a refused call wrote"
            arr[:] = keep
            at = arr.ctypes.data + 4 * s0 - 8 * 3 - gap
            rc = L.gft_debug_mark_spans(*head, b"<", 1, b">", 1, 0, None, 0, at, None, None, None, None)
            assert rc == rc_want, "mark: out_off ending %d bytes below %s[s0]" % (gap, what)
            if rc == 0:
                assert np.frombuffer(C.string_at(at, 24), np.uint64).tolist() == mwant["out_off"] and np.array_equal(arr[s0:], keep[s0:])
            else:
                assert np.array_equal(arr, keep), "a refused call wrote"
            arr[:] = keep
    # the parallel output over the OTHER input array: entries below s0 are not the call's ([s0, s0 + n) of span_rel is written)
    n = int(so[-1]) - s0
    both = np.full(2 * s0 + n + TAIL, R.FULL, np.uint32)
    both[s0 + n:2 * n + s0] = 0                                      # (span_rel = both + n: its entries [s0, s0 + n) lie behind the starts)
    both[s0:s0 + n] = st[s0:s0 + n]
    rc = L.gft_debug_excerpt_spans(blob.ctypes.data, off.ctypes.data, 2, so.ctypes.data, both.ctypes.data, ln.ctypes.data, 2, 2, 0, None, 0, None, None,
                                   None, None, 0, both.ctypes.data + 4 * n, None, None, None)
    assert rc == 0 and both[s0 + n:s0 + 2 * n].tolist() == want["span_rel"][s0:s0 + n] and both[s0:s0 + n].tolist() == st[s0:s0 + n].tolist()
    rc = L.gft_debug_excerpt_spans(blob.ctypes.data, off.ctypes.data, 2, so.ctypes.data, both.ctypes.data, ln.ctypes.data, 2, 2, 0, None, 0, None, None,
                                   None, None, 0, both.ctypes.data + 4 * (n - 1), None, None, None)
    assert rc == _lib.GFT_E_INVALID
    # the map: the two span arrays in one allocation, len's entries below s0 over start's entries behind s0 + n
    docs = ["CAFÉ İ one".encode(), "İİ two Ⱥ".encode()]
    good = [(np.array([0, 2]), np.array([3, 1]))] * 2
    blob, off = TC.pack(docs)
    so, st, ln = LM.flat(good, s0, 0)
    n = 4
    w = LM.expected(docs, good, s0, 0)
    for back, rc_want in ((s0, 0), (s0 + 1, _lib.GFT_E_INVALID)):   # len = start + n + (s0 - back) entries: back == s0 touches, no more
        one = np.full(2 * (s0 + n), R.FULL, np.uint32)
        one[s0:s0 + n] = st[s0:]
        lp = one[n + s0 - back:]
        lp[s0:s0 + n] = ln[s0:]
        if rc_want:
            one[s0:s0 + n] = st[s0:]                                # (the arrays share an entry: whatever it holds, the call is refused)
        keep = one.copy()
        rc = L.gft_debug_map_spans_to_source(blob.ctypes.data, off.ctypes.data, 2, so.ctypes.data, one.ctypes.data, lp.ctypes.data)
        assert rc == rc_want, back
        if rc == 0:
            assert np.array_equal(one[s0:s0 + n], w[1][s0:]) and np.array_equal(lp[s0:s0 + n], w[2][s0:])
        else:
            assert np.array_equal(one, keep)
