"""The four device calls that take "the spans [d_span_off[0], d_span_off[n_docs]) of the caller's span arrays" --
gft_excerpt_spans_device, gft_mark_spans_device, gft_redact_spans_device, gft_map_spans_to_source_device (and gft_map_spans_limit
behind the finder) -- with d_span_off[0] != 0, on one engine, bit for bit against the references of excerpts.py, mark.py, spans.py
and lowermap_cases.py through the checks of span_runs.py that tests/test_span_runs_host.py puts the host walks through: the fixed
cases behind 1, 255, 256 and 257 entries of poison (63, 64, 65 too for the fill) with the text at residues 0, 3 and 15 and both
slack fills; random batches cut at random [a, b) -- doc_off[0] != 0 together with span_off[0] != 0 --; caps that cut the excerpt
list inside a run; one batch past a carry trip behind a base of 257; a run with no spans between runs that have some; partitions
whose runs write into the same parallel arrays; the refusals, after which the handle is usable; the map's limit; and the chain
route -> spans once over the routed blob -> excerpt, mark, redact and map per bucket run.  All comparisons are exact."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (before libgft.so is loaded: one HIP runtime)

import excerpts as X
import lowermap_cases as LM
import mark as M
import span_runs as R
import spans as S
import tolower_cases as TC
from gofindthem_amd import _lib
from gofindthem_amd.engine import Engine, excerpt_shape, lowermap_shape, mark_shape, spans_shape
from gofindthem_amd.finder import EmptyRgxEngine, Finder, GpuEngine

pytestmark = pytest.mark.gpu

L = _lib.load()
XT, XTRIP = excerpt_shape()
BASES = (1, 255, 256, 257)
FILL_BASES = BASES + (63, 64, 65)
RESIDUES = (0, 3, 15)
TAIL = 2


class DeviceMem:
    """span_runs.HostMem's four methods over device tensors of bytes"""

    def put(self, a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()

    def ptr(self, h, at=0):
        return h.data_ptr() + at if h.numel() else None

    def get(self, h):
        return h.cpu().numpy()

    def sync(self):
        torch.cuda.synchronize()


@pytest.fixture(scope="module")
def eng():
    e = Engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def drv(eng):
    limit = L.gft_map_spans_limit                                   # (the finder's entry: declared here, for this module alone)
    limit.restype, limit.argtypes = C.c_int, [C.c_void_p] * 3 + [C.c_uint64] + [C.c_void_p] * 3 + [C.c_uint64]
    calls = {"excerpt": functools.partial(L.gft_excerpt_spans_device, eng._h), "mark": functools.partial(L.gft_mark_spans_device, eng._h),
             "redact": functools.partial(L.gft_redact_spans_device, eng._h), "map": functools.partial(L.gft_map_spans_to_source_device, eng._h),
             "map_limit": functools.partial(limit, eng._h)}
    return R.Driver(DeviceMem(), calls, X, M, S, LM, _lib.GFT_E_INVALID)


def test_the_tiles_are_the_kernels_own():
    assert (XT, mark_shape()[0], spans_shape()[1], lowermap_shape()[3]) == (256, 256, 64, 64)


# ---- the fixed cases behind a base -------------------------------------------------------------------------------------------
def excerpt_cases():
    names = ("gap 0", "the whole document", "a document of no bytes", "documents without spans between", "windows touch in the blob", "no spans at all",
             "a run ends at a tile border", "a run crosses a tile border", "a document border on a tile border", "a later span reaches further back",
             "a lead byte is not the document's", "doc_off[0] != 0")
    by = {c.name: c for c in X.fixed_cases(XT, XTRIP)}
    c = by["documents without spans between"]
    return [by[n] for n in names] + [c.but("documents without spans at the end", docs=c.docs + [b"tail", b""], spans=c.spans + [[], []])]


def mark_cases():
    names = ("run_first_byte", "empty_run_at_ends", "empty_docs", "docs_without_spans", "touch_across_docs", "second_doc_ranks", "no_spans",
             "text_residue_5", "straddle_tile", "many_insertions_in_tile")
    by = {c.name: c for c in M.fixed_cases()}
    c = by["docs_without_spans"]
    return [by[n] for n in names] + M.count_cases(mark_shape()[0], 1024)[:3] + [
        c.but("docs_without_spans_at_both_ends", docs=[b"", c.docs[0]] + c.docs + [c.docs[0], b""], spans=[[], []] + c.spans + [[], []])]


XC, MC = excerpt_cases(), mark_cases()


@pytest.mark.parametrize("i", range(len(XC)), ids=[c.name for c in XC])
def test_excerpt_fixed_cases_behind_a_base(drv, i):
    for j, s0 in enumerate(BASES):
        at = RESIDUES[(i + j) % 3]
        drv.excerpt_case(XC[i], s0, TAIL, fill=0xBF if (i + j) & 1 else 0x00, at=at, shift=(at * 5) % 16)


@pytest.mark.parametrize("i", range(len(MC)), ids=[c.name for c in MC])
def test_mark_fixed_cases_behind_a_base(drv, i):
    for j, s0 in enumerate(BASES):
        at = RESIDUES[(i + j) % 3]
        drv.mark_case(MC[i], s0, TAIL, fill=0x3C if (i + j) & 1 else 0x00, at=at, shift=(at * 5) % 16)


@pytest.mark.parametrize("s0", FILL_BASES)
def test_fill_cases_behind_a_base(drv, s0):
    """every fill case, the refused ones too (every byte as it was): the poison at s0 - 1 and s0 + n is not what refuses them"""
    for i, f in enumerate(S.fill_cases(s0, TAIL)):
        drv.fill_case(f, fill=0x2A if i & 1 else 0x00, at=RESIDUES[(i + s0) % 3])


def map_batches():
    docs, spans = LM.base_docs()
    d130 = [("É%d İ" % i).encode() for i in range(130)]
    return {"base": (docs, spans), "130 documents": (d130, [(np.array([i % 3]), np.array([2])) for i in range(130)]),
            "one document": (docs[:1], spans[:1]), "no spans": (docs, [(np.zeros(0, np.int64),) * 2] * len(docs))}


@pytest.mark.parametrize("name", sorted(map_batches()))
def test_map_batches_behind_a_base(drv, name):
    docs, spans = map_batches()[name]
    for j, s0 in enumerate(BASES + (63, 64, 65)):
        drv.map_case(docs, spans, s0, TAIL, doc_lead=5 * (j & 1), fill=0xC3 if j & 2 else 0x00, at=RESIDUES[j % 3], what=name)


# ---- random batches cut at random [a, b): doc_off[0] != 0 together with span_off[0] != 0 --------------------------------------------
def random_cuts(n_docs, rng, k=2):
    out = []
    for _ in range(k):
        a = int(rng.integers(0, n_docs))
        out.append((a, int(rng.integers(a + 1, n_docs + 1))))
    return out


def test_excerpt_random_batches_cut(drv):
    rng = np.random.default_rng(31)
    for case in X.random_cases():
        want = X.expected(case)
        for a, b in random_cuts(len(case.docs), rng, 1):
            drv.excerpt_cut(case, a, b, want, fill=0xBF if a & 1 else 0x00, at=RESIDUES[a % 3])


def test_mark_random_batches_cut(drv):
    rng = np.random.default_rng(32)
    for case in M.random_cases(6):
        if case.docs:
            want = M.expected(case)
            for a, b in random_cuts(len(case.docs), rng, 1):
                drv.mark_cut(case, a, b, want, at=RESIDUES[a % 3])
    for case in M.count_cases(mark_shape()[0], 1024)[:3]:            # the second document alone: a base of about half a tile
        drv.mark_cut(case, 1, 2, M.expected(case))


def test_fill_random_batches_cut(drv):
    rng = np.random.default_rng(33)
    for f in S.fill_cases():
        if f.ok:
            want = S.redact_reference(f)
            for a, b in random_cuts(len(f.doc_off) - 1, rng, 2):
                drv.fill_cut(f, a, b, want, at=RESIDUES[b % 3])


def test_map_random_batches_cut(drv):
    rng = np.random.default_rng(34)
    docs = TC.random_docs()[:400]
    spans = [LM.every_byte(d, n_random=3, seed=i) if i % 5 else (np.zeros(0, np.int64),) * 2 for i, d in enumerate(docs)]
    for a, b in random_cuts(len(docs), rng, 5) + [(0, 1), (399, 400)]:
        drv.map_case(docs, spans, 0, 0, doc_lead=3, at=RESIDUES[a % 3], a=a, b=b, what="random documents")


def test_a_run_without_spans_between_runs_that_have_some(drv):
    case = next(c for c in XC if c.name == "documents without spans between")      # spans in documents 1 and 4 only
    assert [len(s) for s in case.spans] == [0, 1, 0, 0, 2]
    want = X.expected(case, None, 256, TAIL)
    for a, b in ((2, 4), (0, 1), (2, 3)):
        drv.excerpt_cut(case, a, b, want, 256, TAIL)
    drv.excerpt_partition(case, [(0, 2), (2, 4), (4, 5)], want, 256, TAIL)
    mc = M.Case(case.name, case.docs, case.spans)
    mwant = M.expected(mc, None, 256, TAIL)
    drv.mark_cut(mc, 2, 4, mwant, 256, TAIL)
    drv.mark_partition(mc, [(0, 2), (2, 4), (4, 5)], mwant, 256, TAIL)
    f = S.fill_case("no spans between", [20, 20, 30, 5, 25], case.spans, seed=5, lead=3, span_lead=64, span_tail=TAIL)
    drv.fill_cut(f, 2, 4, S.redact_reference(f))
    drv.fill_partition(f, [(0, 2), (2, 4), (4, 5)])


# ---- caps and count-only calls under a base ----------------------------------------------------------------------------------------
def test_caps_that_cut_the_excerpt_list_inside_a_run(drv):
    """exc_span_off[cap] holds an index into the caller's arrays, whatever the cap; count-only calls with NULL outputs count the run"""
    case = next(c for c in XC if c.name == "a run crosses a tile border")
    whole = case.but("three of them", docs=case.docs * 3, spans=case.spans * 3)
    arrays = whole.arrays(0xBF, 257, TAIL)
    want = R.restrict(R.Whole("excerpt", arrays, X.expected(whole, None, 257, TAIL)), 1, 3)
    m, total = want["n_exc"], want["total"]
    assert m >= 4 and int(arrays[2][1]) > 257 + XT
    bt = R.Batch(drv.mem, arrays, 0xBF, 3)
    rc, r = R.run_excerpt(drv.calls["excerpt"], bt, 1, 3, case.before, case.after, 1, None, count_only=True)
    assert rc == 0 and (r["n_exc"], r["total"]) == (m, total)
    for cap in (m - 1, m // 2, 1, 0):
        rel = R.Out(drv.mem, bt.n_entries, np.uint32)
        rc, r = R.run_excerpt(drv.calls["excerpt"], bt, 1, 3, case.before, case.after, 1, rel, cap_exc=cap, shift=5)
        assert rc == 0 and (r["n_exc"], r["total"]) == (m, total), cap
        assert r["exc_span_off"] == want["exc_span_off"][:cap + 1] and r["exc_off"] == want["exc_off"][:cap + 1], cap
        assert r["exc_doc"] == want["exc_doc"][:cap] and r["exc_start"] == want["exc_start"][:cap], cap
        assert r["doc_exc_off"] == want["doc_exc_off"] and r["out"] == want["out"], cap
        R.parallel(rel, want["span_rel"], "span_rel")
    mc = M.Case("three of them", whole.docs, whole.spans)
    mwant = R.restrict(R.Whole("mark", arrays, M.expected(mc, None, 257, TAIL)), 1, 3)
    rc, r = R.run_mark(drv.calls["mark"], bt, 1, 3, mc.open, mc.close, None, count_only=True)
    assert rc == 0 and (r["n_runs"], r["total"]) == (mwant["n_runs"], mwant["total"])
    new = R.Out(drv.mem, bt.n_entries, np.uint32)
    rc, r = R.run_mark(drv.calls["mark"], bt, 1, 3, mc.open, mc.close, new, cap_bytes=mwant["total"] // 2)
    assert rc == 0 and r["out"] == mwant["out"][:mwant["total"] // 2] and r["out_off"] == mwant["out_off"]
    R.parallel(new, mwant["span_new"], "span_new")


def test_past_a_carry_trip_behind_a_base_of_257(drv):
    """more than 256 x 1024 spans behind 257 entries of poison: the carry's second trip meets the base"""
    case = next(c for c in X.fixed_cases(XT, XTRIP) if c.name == "a second carry trip")
    assert sum(len(s) for s in case.spans) == XT * XTRIP + 1
    drv.excerpt_case(case, 257, TAIL, fill=0xBF, at=3)
    mc = M.count_cases(mark_shape()[0], 1024)[3]
    assert sum(len(s) for s in mc.spans) == XT * XTRIP + 1 and len(mc.docs) == 2
    drv.mark_case(mc, 257, TAIL, fill=0x3C, at=15)
    drv.mark_cut(mc, 1, 2, M.expected(mc, None, 257, TAIL), 257, TAIL)        # the second document alone: a base of half the batch


# ---- partitions ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def thousands():
    """3 000 short documents, 0 .. 4 spans each: an excerpt case, and the same documents and spans as a mark case"""
    rng = np.random.default_rng(41)
    docs, spans = [], []
    for _ in range(3000):
        doc = b"".join(X.ALPHABET[int(k)] for k in rng.integers(0, len(X.ALPHABET), int(rng.integers(0, 50))))
        ends = np.sort(rng.integers(0, len(doc) + 1, int(rng.integers(0, 5)) if rng.random() < 0.7 else 0))
        docs.append(doc)
        spans.append([(e - min(e, k), min(e, k)) for e, k in zip(ends.tolist(), rng.integers(0, 6, ends.size).tolist())])
    return X.Case("3 000 documents", docs, spans, 5, 7, True, lead=2), M.Case("3 000 documents", docs, spans, b"<b>", b"</b>", lead=2)


def test_partitions_of_a_few_thousand_documents(drv):
    rng = np.random.default_rng(42)
    xc, mc = thousands()
    xw, mw = X.expected(xc, None, 255, TAIL), M.expected(mc, None, 255, TAIL)
    for parts in (1, 2, 3, 7):
        drv.excerpt_partition(xc, R.partition(3000, parts, rng), xw, 255, TAIL, at=3)
        drv.mark_partition(mc, R.partition(3000, parts, rng), mw, 255, TAIL, at=15)
    f = next(f for f in S.fill_cases(65, TAIL) if f.name == "random: 3 000 documents")
    for parts in (1, 2, 3, 7):
        drv.fill_partition(f, R.partition(3000, parts, rng), at=3)
    docs = TC.random_docs()[:2000]
    spans = [LM.every_byte(d, n_random=2, seed=i) if i % 3 else (np.zeros(0, np.int64),) * 2 for i, d in enumerate(docs)]
    for parts in (1, 3, 7):
        drv.map_partition(docs, spans, R.partition(2000, parts, rng), 63, TAIL, doc_lead=1)


def test_partitions_into_runs_of_one_document(drv):
    rng = np.random.default_rng(43)
    for case in XC:
        if len(case.docs) <= 40:
            want = X.expected(case, None, 3, TAIL)
            for p in sorted({1, 2, 3, len(case.docs)} & set(range(1, len(case.docs) + 1))):
                drv.excerpt_partition(case, R.partition(len(case.docs), p, rng), want, 3, TAIL)
    for case in MC:
        want = M.expected(case, None, 3, TAIL)
        for p in sorted({1, 2, 3, len(case.docs)} & set(range(1, len(case.docs) + 1))):
            drv.mark_partition(case, R.partition(len(case.docs), p, rng), want, 3, TAIL)
    docs, spans = LM.base_docs()
    drv.map_partition(docs, spans, R.partition(len(docs), len(docs), rng), 5, TAIL, doc_lead=2)
    f = S.fill_case("six documents", [30] * 6, [[(1, 2)], [], [(0, 30), (5, 1)], [], [(29, 1)], [(3, 3)]], seed=8, lead=1, span_lead=5, span_tail=TAIL)
    drv.fill_partition(f, R.partition(6, 6, rng))


# ---- refusals under a base: nothing was written, the handle stays usable, the next correct call is right ----------------------------
def test_refusals_under_a_base(drv):
    body = X._rand_bytes(60, 3)
    good = [[(2, 3), (10, 2), (30, 5)], [(1, 1), (20, 4)]]
    first_past = [[(58, 3), (59, 1), (59, 1)], good[1]]            # index s0: start + len = 61 > 60, the ends still ascending
    last_past = [good[0], [(1, 1), (57, 4)]]                       # index s0 + n - 1
    descend = [[(2, 9), (3, 2), (30, 5)], good[1]]                 # end 11 at s0, end 5 at s0 + 1
    ok, okm = X.Case("good", [body, body], good, 2, 2), M.Case("good", [body, body], good)
    for s0 in (1, 256):
        for what, spans in (("past at s0", first_past), ("past at s0 + n - 1", last_past), ("ends descend at s0", descend)):
            drv.excerpt_refused(X.Case(what, [body, body], spans, 2, 2), s0, TAIL, what=what)
            drv.excerpt_case(ok, s0, TAIL)
            drv.mark_refused(M.Case(what, [body, body], spans), s0, TAIL, what=what)
            drv.mark_case(okm, s0, TAIL)
        for so, what in (([s0 + 5, s0 + 3, s0], "span_off[n_docs] < span_off[0]"), ([s0, s0 + 4, s0 + 3], "span offsets descend")):
            drv.excerpt_refused(ok, s0, TAIL, so=so, what=what)
            drv.excerpt_case(ok, s0, TAIL)
            drv.mark_refused(okm, s0, TAIL, so=so, what=what)
            drv.mark_case(okm, s0, TAIL)
    for s0 in (1, 64):
        f = S.fill_case("good", [40, 40], [[(0, 4)], [(5, 5)]], seed=4, span_lead=s0, span_tail=TAIL)
        for spans, what in (([[(38, 3), (0, 1)], [(5, 5)]], "past at s0"), ([[(0, 4)], [(5, 5), (36, 5)]], "past at s0 + n - 1")):
            drv.fill_refused(S.fill_case(what, [40, 40], spans, seed=3, lead=2, span_lead=s0, span_tail=TAIL), what)
            drv.fill_case(f)
        drv.fill_refused(f._replace(span_off=np.array([s0 + 2, s0 + 1, s0], np.uint64)), "span_off[n_docs] < span_off[0]")
        drv.fill_case(f)
    docs = ["CAFÉ İ one".encode(), "İİ two Ⱥ".encode()]
    Bs = [LM.lowered_len(d) for d in docs]
    good = [(np.array([0, 2]), np.array([3, 1]))] * 2
    for s0 in (1, 64):
        for bad, what in (([(np.array([Bs[0] - 1, 1]), np.array([2, 1])), (np.array([0]), np.array([1]))], "past at s0"),
                          ([(np.array([0]), np.array([1])), (np.array([1, Bs[1]]), np.array([1, 1]))], "past at s0 + n - 1")):
            drv.map_refused(docs, *LM.flat(bad, s0, TAIL), what=what)
            drv.map_case(docs, good, s0, TAIL, what="good")
        so, st, ln = LM.flat(good, s0, TAIL)
        drv.map_refused(docs, [s0 + 4, s0 + 2, s0], st, ln, what="span_off[n_docs] < span_off[0]")
        drv.map_case(docs, good, s0, TAIL, what="good")


def test_overlap_checks_under_a_base(drv, eng):
    """an output that overlaps only entries below s0 of a span array is no overlap; one that overlaps one entry inside is"""
    s0 = 40
    body = X._rand_bytes(60, 5)
    case = X.Case("overlap", [body, body], [[(2, 3), (10, 2)], [(1, 1), (20, 4)]], 2, 2, runes=False)
    want = X.expected(case, None, s0, TAIL)
    mwant = M.expected(M.Case("overlap", case.docs, case.spans, b"<", b">"), None, s0, TAIL)
    m = want["n_exc"]
    bt = R.Batch(drv.mem, case.arrays(0, s0, TAIL))
    for h, what in ((bt.st, "span_start"), (bt.ln, "span_len")):
        for gap, rc_want in ((0, 0), (-4, _lib.GFT_E_INVALID)):
            keep = h.clone()
            at = h.data_ptr() + 4 * s0 - 8 * (m + 1) - gap
            torch.cuda.synchronize()
            rc = drv.calls["excerpt"](*bt.args(), 2, 2, 0, None, 0, at, None, None, None, m, None, None, None, None)
            assert rc == rc_want, "excerpt: exc_off ending %d bytes below %s[s0]" % (gap, what)
            got = h.cpu().numpy()
            if rc == 0:
                lo = 4 * s0 - 8 * (m + 1)
                assert got[lo:4 * s0].view(np.uint64).tolist() == want["exc_off"] and (got[4 * s0:] == keep.cpu().numpy()[4 * s0:]).all()
            else:
                assert (got == keep.cpu().numpy()).all(), "a refused call wrote"
            h.copy_(keep)
            at = h.data_ptr() + 4 * s0 - 8 * 3 - gap
            torch.cuda.synchronize()
            rc = drv.calls["mark"](*bt.args(), b"<", 1, b">", 1, 0, None, 0, at, None, None, None, None)
            assert rc == rc_want, "mark: out_off ending %d bytes below %s[s0]" % (gap, what)
            got = h.cpu().numpy()
            if rc == 0:
                assert got[4 * s0 - 24:4 * s0].view(np.uint64).tolist() == mwant["out_off"] and (got[4 * s0:] == keep.cpu().numpy()[4 * s0:]).all()
            else:
                assert (got == keep.cpu().numpy()).all(), "a refused call wrote"
            h.copy_(keep)
    drv.excerpt_case(case, s0, TAIL)


# ---- the map's limit: an index into the caller's arrays ------------------------------------------------------------------------------
def test_the_maps_limit_under_a_base(drv):
    docs, spans = LM.base_docs()
    n = sum(len(s) for s, _ in spans)
    for s0 in (1, 64, 65):
        for limit in (0, s0 - 1, s0, s0 + 1, s0 + n // 2, s0 + n - 1, s0 + n, s0 + n + 1, s0 + n + TAIL + 9):
            drv.map_case(docs, spans, s0, TAIL, doc_lead=2, limit=limit, what="limit")
    # ... and over a run cut from the batch: the limit still counts from the arrays' first entry
    so = LM.flat(spans, 3, TAIL)[0]
    for limit in (int(so[2]) - 1, int(so[2]), int(so[2]) + 4, int(so[5]), int(so[5]) + 1):
        drv.map_case(docs, spans, 3, TAIL, limit=limit, a=2, b=5, what="limit over a run")


# ---- the chain: route, spans once over the routed blob, then every bucket run on its own -----------------------------------------
LOG = [b"GET /index.html 200", b"POST /login 401 bad password for root", b"GET /admin 403", b"kernel: oom-killer invoked", b"",
       b"POST /login 200 root", b"GET /health 200", b"sshd: Failed password for root from 10.0.0.7", b"cron: job done"] * 3
LOG_EXPRS = ['"password" and "root"', '"403" or "oom"', '"GET" and not "200"', 'inord("POST" and "login")', '"café" or "ÿ"', '"ⱥ"']
BUCKETS = [[0], [1], [2], [3], [4], [5]]                            # ("ⱥ" is the lower-case form of U+023A, one byte longer: its spans shrink)


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


def routed(finder, lines, source=False):
    """route the lines, then the spans ONCE over the whole routed blob -> the device tensors and their host copies"""
    data = b"".join(lines)
    out, out_off, doc_idx, bucket_doc, _, _, bm = finder.RouteLinesDevice(resident(data), len(data), BUCKETS)
    so, st, ln, _, low = finder.SpansDevice(out, out_off, bm, row_idx=doc_idx, source=source)
    assert int(so[0]) == 0
    off = out_off.cpu().numpy().astype(np.uint64)
    docs = [lines[i] for i in doc_idx.cpu().tolist()]
    assert out.cpu().numpy().tobytes()[:int(off[-1])] == b"".join(docs)
    h = {"off": off, "so": so.cpu().numpy().astype(np.uint64), "st": st.cpu().numpy().view(np.uint32), "ln": ln.cpu().numpy().view(np.uint32)}
    return (out, out_off, so, st, ln, low), h, docs, bucket_doc.tolist() if hasattr(bucket_doc, "tolist") else list(bucket_doc)


def per_doc(h, n):
    so = h["so"].astype(np.int64)
    return [list(zip(h["st"][so[d]:so[d + 1]].tolist(), h["ln"][so[d]:so[d + 1]].tolist())) for d in range(n)]


def test_chain_route_spans_then_every_bucket_run(finder):
    lines = [ln + b"\n" for ln in LOG]
    (out, out_off, so, st, ln, low), h, docs, bucket_doc = routed(finder, lines)
    assert not low and len(bucket_doc) == len(BUCKETS) + 1
    spans = per_doc(h, len(docs))
    blob = np.frombuffer(out.cpu().numpy().tobytes(), np.uint8)
    arrays = (blob, h["off"], h["so"], h["st"], h["ln"])
    xwhole = R.Whole("excerpt", arrays, X.expected(X.Case("routed", docs, spans, 6, 4)))
    mwhole = R.Whole("mark", arrays, M.expected(M.Case("routed", docs, spans, b"**", b"**")))
    f = S.FillCase("routed", blob, h["off"], h["so"], h["st"], h["ln"], ord("#"), True)
    rwhole = R.Whole("redact", arrays, S.redact_reference(f))
    based = 0
    for b0, b1 in zip(bucket_doc, bucket_doc[1:]):
        if b1 == b0:
            continue
        based += int(h["so"][b0]) != 0 and int(h["so"][b1]) > int(h["so"][b0])
        run_off, run_so = out_off[b0:b1 + 1].contiguous(), so[b0:b1 + 1].contiguous()
        t = finder.ExcerptsDevice(out, run_off, run_so, st, ln, low, False, 6, 4)
        got = {"n_exc": int(t[2].numel()), "total": int(t[0].numel()), "out": t[0].cpu().numpy().tobytes()}
        got.update({k: v.cpu().numpy().tolist() for k, v in zip(X.ARRAYS, t[1:7])})
        d = R.differs(got, R.restrict(xwhole, b0, b1), 0)           # (ExcerptsDevice hands span_rel back zeroed where it is not written)
        assert d is None, "excerpts of the bucket run [%d, %d): %s" % (b0, b1, d)
        t = finder.MarkDevice(out, run_off, run_so, st, ln, low, False, b"**", b"**")
        got = {"n_runs": int(t[3][-1]), "total": int(t[0].numel()), "out": t[0].cpu().numpy().tobytes(), "out_off": t[1].cpu().numpy().tolist(),
               "span_new": t[2].cpu().numpy().tolist(), "doc_run_off": t[3].cpu().numpy().tolist()}
        d = R.differs(got, R.restrict(mwhole, b0, b1), 0)
        assert d is None, "marks of the bucket run [%d, %d): %s" % (b0, b1, d)
        masked = out.clone()
        torch.cuda.synchronize()
        assert L.gft_redact_spans_device(finder.engine_handle(), masked.data_ptr(), run_off.data_ptr(), b1 - b0, run_so.data_ptr(), st.data_ptr(),
                                         ln.data_ptr(), ord("#")) == 0
        assert masked.cpu().numpy().tobytes() == R.restrict(rwhole, b0, b1), "redaction of the bucket run [%d, %d)" % (b0, b1)
    assert based >= 2, "the buckets behind the first hold spans: the runs have a base"


def test_chain_route_spans_then_the_map_per_bucket_run_of_a_lowered_batch(finder):
    lines = [ln + b"\n" for ln in LOG]
    lines[2] = "GET /CAFÉ 403 Ÿ oom\n".encode()
    lines[3] = "KERNEL: OOM-killer İnvoked by CAFÉ 403\n".encode()        # U+0130 shrinks: what follows moves to the left
    lines[6] = "Ⱥ grows, then a PASSWORD for root ⱥⱥⱥ café\n".encode()     # U+023A grows: what follows moves to the right
    lines[7] = b"\x80 oom behind a lone continuation byte 403\n"           # an invalid byte becomes three
    (out, out_off, so, st, ln, low), h, docs, bucket_doc = routed(finder, lines)
    assert low
    n = len(docs)
    so64 = h["so"].astype(np.int64)
    spans = [(h["st"][so64[d]:so64[d + 1]].astype(np.int64), h["ln"][so64[d]:so64[d + 1]].astype(np.int64)) for d in range(n)]
    w = LM.expected(docs, spans)
    assert w is not None and (w[1] != h["st"]).any() and (w[2] != h["ln"]).any(), "the map moves spans and changes lengths"
    arrays = (None, h["off"], h["so"], h["st"].copy(), h["ln"].copy())
    done = 0
    for b0, b1 in zip(bucket_doc, bucket_doc[1:]):
        if b1 == b0:
            continue
        run_off, run_so = out_off[b0:b1 + 1].contiguous(), so[b0:b1 + 1].contiguous()
        torch.cuda.synchronize()
        assert L.gft_map_spans_to_source_device(finder.engine_handle(), out.data_ptr(), run_off.data_ptr(), b1 - b0, run_so.data_ptr(), st.data_ptr(),
                                                ln.data_ptr()) == 0
        want = R.restrict(R.Whole("map", arrays, w[1:]), b0, b1)    # this run mapped, every other entry as the runs before left it
        got = (st.cpu().numpy().view(np.uint32), ln.cpu().numpy().view(np.uint32))
        d = R.differs(got, want)
        assert d is None, "the map of the bucket run [%d, %d): %s" % (b0, b1, d)
        arrays = arrays[:3] + (want[0], want[1])
        done += int(so64[b1] > so64[b0] and so64[b0] > 0)
    assert done >= 2 and np.array_equal(arrays[3], w[1]) and np.array_equal(arrays[4], w[2])
    # the finder's own route (gft_map_spans_limit behind SpansDevice(source=True)) gives the same spans
    (_, _, so2, st2, ln2, low2), h2, _, _ = routed(finder, lines, source=True)
    assert low2 and np.array_equal(h2["so"], h["so"]) and np.array_equal(h2["st"], w[1]) and np.array_equal(h2["ln"], w[2])
    # ... and the mapped spans redact the caller's bytes, bucket run by bucket run
    blob = np.frombuffer(out.cpu().numpy().tobytes(), np.uint8)
    f = S.FillCase("routed", blob, h["off"], h["so"], w[1], w[2], ord("#"), True)
    masked = out.clone()
    for b0, b1 in zip(bucket_doc, bucket_doc[1:]):
        if b1 > b0:
            run_off, run_so = out_off[b0:b1 + 1].contiguous(), so[b0:b1 + 1].contiguous()
            torch.cuda.synchronize()
            assert L.gft_redact_spans_device(finder.engine_handle(), masked.data_ptr(), run_off.data_ptr(), b1 - b0, run_so.data_ptr(), st.data_ptr(),
                                             ln.data_ptr(), ord("#")) == 0
    assert masked.cpu().numpy().tobytes() == S.redact_reference(f)
