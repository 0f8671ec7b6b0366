"""Term statistics and column counts on the device (csrc/gft_stats.hip): gft_term_stats_device and gft_count_columns_device against
the numpy reference of term_stats.py on the cases test_term_stats_host.py runs through the host walk -- the borders of the walk from
gft_debug_stats_shape, the accumulation, the 64-bit carry, every output NULL on its own, the refusals, which leave the counters
byte for byte and the handle usable, the overlaps, a handful of seeded Zipf lists --, the calls behind the scan and the spans, and
the finder layer end to end: TermStatsLines against counts made from SpansLines' own output and from the oracle's match list, with
a batch that is lowered; CountExpressions against the column sums of ProcessLines' rows and against CountLines.  All comparisons
are exact."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest
import torch  # noqa: F401  (before libgft.so is loaded: one HIP runtime)

import term_stats as TS
from gofindthem_amd import _lib
from gofindthem_amd.engine import Engine, pack, stats_shape
from gofindthem_amd.finder import EmptyRgxEngine, Finder, FinderError, GpuEngine, PyRegexpEngine
from oracle.pyoracle import Oracle, pack_strings

pytestmark = pytest.mark.gpu

SH = stats_shape()
FIXED = TS.fixed_cases(SH)
RANDOM = TS.random_cases(SH, 6, seed=99)
COLUMNS = TS.column_cases(SH)
REFUSALS = TS.refusal_inputs(SH)


@pytest.fixture(scope="module")
def eng():
    e = Engine()
    yield e
    e.close()


def dev(a):
    """a numpy array of 32- or 64-bit words on the device (None stays None; an empty one gets a word, so that it has an address)"""
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    signed = a.view(np.int64 if a.dtype.itemsize == 8 else np.int32)
    return torch.from_numpy(np.concatenate([signed.ravel(), np.zeros(1, signed.dtype)])).cuda()[:a.size]


def ptr(t):
    return t.data_ptr() if t is not None else None


def runner(e):
    def run(off, term, n_docs, n_terms, flags, doc_base, occ, docs, first):
        d_off, d_term = dev(off), dev(term)
        outs = [dev(a) for a in (occ, docs, first)]
        torch.cuda.synchronize()
        rc = _lib.load().gft_term_stats_device(e._h, ptr(d_off) if n_docs else None, ptr(d_term), n_docs, n_terms, flags, doc_base,
                                               *(ptr(o) for o in outs))
        torch.cuda.synchronize()
        for a, o in zip((occ, docs, first), outs):
            if a is not None:
                a[:] = o.cpu().numpy().view(np.uint64)
        return rc
    return run


def cols_runner(e):
    def run_cols(bm, n_rows, n_cols, row_idx, flags, count):
        d_bm, d_idx, d_count = dev(bm), dev(row_idx), dev(count)
        torch.cuda.synchronize()
        rc = _lib.load().gft_count_columns_device(e._h, ptr(d_bm) if bm.size else None, n_rows, n_cols,
                                                  ptr(d_idx) if row_idx is not None and len(row_idx) else None, flags, ptr(d_count))
        torch.cuda.synchronize()
        count[:] = d_count.cpu().numpy().view(np.uint64)
        return rc
    return run_cols


def test_symbols_present():
    L = _lib.load()
    for name in ("gft_term_stats_device", "gft_count_columns_device", "gft_batch_term_stats_device", "gft_finder_term_stats_device",
                 "gft_debug_stats_shape"):
        assert hasattr(L, name) and name in _lib.SYMBOLS


@pytest.mark.parametrize("case", FIXED, ids=[c.name for c in FIXED])
def test_fixed(eng, case):
    TS.check_case(runner(eng), case, doc_base=(1 << 40) + 3)


@pytest.mark.parametrize("case", RANDOM, ids=[c.name for c in RANDOM])
def test_random(eng, case):
    TS.check_case(runner(eng), case, doc_base=12345)


def test_null_outputs(eng):
    for case in FIXED[:2] + RANDOM[:1]:
        TS.check_null_outputs(runner(eng), case)


@pytest.mark.parametrize("name", ["step_sum_%d" % SH["step_entries"], "ranges", "large_between_small", "cut_middle"])
def test_accumulate_halves(eng, name):
    case = next(c for c in FIXED if c.name == name)
    for cut in sorted({0, case.n_docs // 2, case.n_docs}):
        TS.check_accumulate_halves(runner(eng), case, cut)


def test_accumulate_carry(eng):
    TS.check_accumulate_carry(runner(eng))


@pytest.mark.parametrize("r", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(eng, r):
    TS.check_refusal(runner(eng), *r[1:])
    TS.check_case(runner(eng), FIXED[0])                            # the handle stays usable


def test_overlaps(eng):
    """an output that overlaps an input or another output: refused, nothing written"""
    L = _lib.load()
    case = next(c for c in FIXED if c.name == "cut_middle")
    nt, n = case.n_terms, case.n_docs
    d_off, d_term = dev(case.off), dev(case.term)
    pool = torch.full((4 * nt,), 0x77, dtype=torch.int64, device="cuda")
    w = 8
    p = pool.data_ptr()
    sets = {"same": (p, p, p + 2 * nt * w), "occ_docs": (p, p + (nt - 1) * w, p + 2 * nt * w), "docs_first": (p, p + nt * w, p + (2 * nt - 1) * w),
            "occ_first": (p + w, None, p), "offsets": (None, d_off.data_ptr() + 3 * w, None),
            "entries": (None, None, d_term.data_ptr() + 778 * 4)}
    keep_off, keep_term = d_off.clone(), d_term.clone()
    for name, (a, b, c) in sets.items():
        torch.cuda.synchronize()
        assert L.gft_term_stats_device(eng._h, d_off.data_ptr(), d_term.data_ptr(), n, nt, 0, 0, a, b, c) == TS.E_INVALID, name
        assert bool((pool == 0x77).all()) and torch.equal(d_off, keep_off) and torch.equal(d_term, keep_term), name
    # (the entries in front of off[0] are no input: an output there is fine)
    assert L.gft_term_stats_device(eng._h, d_off.data_ptr(), d_term.data_ptr(), n, nt, 0, 0, d_term.data_ptr(), None, None) == 0
    bm = torch.full((8, 2), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert L.gft_count_columns_device(eng._h, bm.data_ptr(), 8, 6, None, 0, bm.data_ptr() + 16) == TS.E_INVALID and bool((bm == -1).all())
    idx = torch.arange(40, dtype=torch.int64, device="cuda") % 8
    torch.cuda.synchronize()
    assert L.gft_count_columns_device(eng._h, bm.data_ptr(), 40, 40, idx.data_ptr(), 0, idx.data_ptr()) == TS.E_INVALID
    assert idx.tolist() == [k % 8 for k in range(40)]


@pytest.mark.parametrize("c", COLUMNS, ids=[c[0] for c in COLUMNS])
def test_columns(eng, c):
    TS.check_columns(cols_runner(eng), *c)


def test_engine_wrappers_and_profile_names(eng):
    case = next(c for c in FIXED if c.name == "ranges")
    want = TS.reference(case.off, case.term, case.n_docs, case.n_terms, 50)
    eng.profile(True)
    eng.profile_reset()
    try:
        occ, docs, first = eng.term_stats_device(dev(case.off), dev(case.term), case.n_docs, case.n_terms, doc_base=50)
        name, bm, n_cols, idx = next(c for c in COLUMNS if c[0] == "row_idx_long")
        count = eng.count_columns_device(dev(bm).reshape(bm.shape), n_cols, dev(idx))
        for cat in ("stats_check", "stats_count", "stats_columns"):
            assert eng.profile_read(cat)[1] == 1, cat
    finally:
        eng.profile(False)
    for g, w in zip((occ, docs, first), want):
        assert (g.cpu().numpy().view(np.uint64) == w).all()
    assert (count.cpu().numpy().view(np.uint64) == TS.columns_reference(bm, n_cols, idx)).all()
    # accumulate into what came back: twice the counts, the first document of the earlier batch stays
    occ2, docs2, first2 = eng.term_stats_device(dev(case.off), dev(case.term), case.n_docs, case.n_terms, occ, docs, first, accumulate=True,
                                                doc_base=9000)
    assert occ2 is occ and (occ.cpu().numpy().view(np.uint64) == 2 * want[0]).all() and (first.cpu().numpy().view(np.uint64) == want[2]).all()
    count2 = eng.count_columns_device(dev(bm).reshape(bm.shape), n_cols, dev(idx), count=count, accumulate=True)
    assert (count2.cpu().numpy().view(np.uint64) == 2 * TS.columns_reference(bm, n_cols, idx)).all()


TEXTS = [b"the cat sat on the mat with the hat", b"", b"a cat, a hat and a bat", b"no match here", b"the the the the", b"hat" * 50] * 30
TERMS = [b"the", b"cat", b"hat", b"at", b"mat", b"zebra"]


def test_behind_the_scan(eng):
    """(match_off, term_id) of scan_device, with and without GFT_SCAN_UNIQUE, as the call takes them; gft_last_nonascii is left alone"""
    eng.build(TERMS)
    blob, off = pack(TEXTS)
    text = torch.from_numpy(np.concatenate([blob, np.zeros(64, np.uint8)])).cuda()
    d_off = dev(off)
    torch.cuda.synchronize()
    for unique in (False, True):
        mo, ti, _ = eng.scan(blob, off, unique=unique)
        want = TS.reference(mo, ti, len(TEXTS), eng.n_terms)
        m = eng.scan_device(text.data_ptr(), d_off.data_ptr(), len(TEXTS), unique=unique)
        before = _lib.load().gft_last_nonascii(eng._h)
        got = eng.term_stats_device(m.match_off, m.term_id, len(TEXTS), eng.n_terms)
        assert _lib.load().gft_last_nonascii(eng._h) == before
        for g, w in zip(got, want):
            assert (g.cpu().numpy().view(np.uint64) == w).all()
        if unique:
            assert (want[0] == want[1]).all()                       # every term once a document
    # the whole batch in one call: every dictionary match
    occ, docs, first = (torch.zeros(eng.n_terms, dtype=torch.int64, device="cuda") for _ in range(3))
    torch.cuda.synchronize()
    again = C.c_int(5)
    assert _lib.load().gft_batch_term_stats_device(eng._h, text.data_ptr(), d_off.data_ptr(), len(TEXTS), 0, None, None, 0, 0, occ.data_ptr(),
                                                   docs.data_ptr(), first.data_ptr(), C.byref(again)) == 0 and again.value == 0
    mo, ti, _ = eng.scan(blob, off)
    for g, w in zip((occ, docs, first), TS.reference(mo, ti, len(TEXTS), eng.n_terms)):
        assert (g.cpu().numpy().view(np.uint64) == w).all()


LOG = [b"GET /index.html 200", b"POST /login 401 bad password for root", b"GET /admin 403", b"kernel: oom-killer invoked", b"",
       b"POST /login 200 root", b"GET /health 200", b"sshd: Failed password for root from 10.0.0.7", b"cron: job done password password"] * 40
LOG_EXPRS = [('"password" and "root"', "auth"), ('"403" or "oom"', "alert"), ('"GET" and not "200"', "alert"), ('inord("POST" and "login")', "auth"),
             ('"cron"', "")]


def log_finder():
    f = Finder(GpuEngine.__new__(GpuEngine), EmptyRgxEngine(), False)
    for e, t in LOG_EXPRS:
        f.AddExpressionWithTag(e, t)
    return f


def to_lower(b):
    out = np.zeros(3 * len(b) + 1, dtype=np.uint8)
    n = C.c_uint64(0)
    assert _lib.load().gft_to_lower(b, len(b), out.ctypes.data, out.size, C.byref(n)) == 0
    return out[:n.value].tobytes()


@pytest.mark.parametrize("lowered", [False, True])
def test_finder_term_stats_lines(lowered):
    lines = [ln + b"\n" for ln in LOG]
    if lowered:
        lines[3] = "KERNEL: OOM-killer invoked by CAFÉ root PASSWORD\n".encode()
    data = b"".join(lines)
    f = log_finder()
    try:
        # the kept matches: counted in Python from what SpansLines lists
        for want in (None, f.want_mask([0, 4]), f.want_mask(tags=["alert"])):
            idx, spans, low = f.SpansLines(data, want)
            occ, docs, first = Counter(), Counter(), {}
            for d, sp in zip(idx.tolist(), spans):
                for t in [s[2] for s in sp]:
                    occ[t] += 1
                for t in {s[2] for s in sp}:
                    docs[t] += 1
                    first.setdefault(t, d)
            got, low2 = f.TermStatsLines(data, want)
            assert low == low2 == lowered
            assert got == {t: (occ[t], docs[t], first[t]) for t in occ} and got
        # every dictionary match: the oracle's list over the text the finder scans
        kw = sorted(k.encode() for k in f.GetKeywords())
        orc = Oracle(kw)
        names = orc.terms()
        blob, off = pack_strings([to_lower(ln) for ln in lines])
        mo, ti, _ = orc.scan(blob, off, fold=False)
        o, d, fi = TS.reference(mo, ti, len(lines), orc.n_terms)
        want_all = {names[t]: (int(o[t]), int(d[t]), int(fi[t])) for t in range(orc.n_terms) if o[t]}
        got, low = f.TermStatsLines(data, kept=False)
        assert got == want_all and low == lowered and b"200" in got     # ("200" is under a NOT only: never kept, always counted here)
        assert b"200" not in f.TermStatsLines(data)[0]
        # accumulation over two batches, nothing coming down in between
        buf = f._resident(data)
        doc_off = f.SplitLinesDevice(buf, len(data), 0)
        n = int(doc_off.numel()) - 1
        acc = f.TermStatsDevice(buf, doc_off)[:3]
        acc2 = f.TermStatsDevice(buf, doc_off, accumulate_into=acc, doc_base=n)
        assert acc2[0] is acc[0] and acc2[3] == lowered
        eng_terms = {}
        tp, tl = C.c_void_p(), C.c_uint32()
        for t in range(int(acc[0].numel())):
            assert _lib.load().gft_term(f.engine_handle(), t, C.byref(tp), C.byref(tl)) == 0
            eng_terms[t] = C.string_at(tp.value, tl.value)
        occ, docs, first = (a.cpu().numpy() for a in acc)
        assert {eng_terms[t]: (int(occ[t]), int(docs[t]), int(first[t])) for t in np.nonzero(occ)[0].tolist()} == \
            {k: (2 * v[0], 2 * v[1], v[2]) for k, v in want_all.items()}
    finally:
        f.close()


def test_finder_count_expressions():
    data = b"".join(ln + b"\n" for ln in LOG)
    f = log_finder()
    try:
        count = f.CountExpressions(data)
        _, rows = f.ProcessLines(data)
        E = f.n_expressions
        assert count.dtype == np.uint64 and count.tolist() == TS.columns_reference(rows, E).tolist() and count.all()
        # per tag: the lines CountLines gives the tag's bucket are the lines on which any of its expressions is true
        tags = ["auth", "alert"]
        docs, _ = f.CountLines(data, tags)
        for k, tag in enumerate(tags):
            w = f.want_mask(tags=[tag])
            assert int(docs[k]) == int((rows & w[None, :]).any(axis=1).sum())
            mine = [i for i in range(E) if int(w[i // 32]) >> (i % 32) & 1]
            assert max(int(count[i]) for i in mine) <= int(docs[k]) <= sum(int(count[i]) for i in mine)
        # a tag of one expression: the two calls agree exactly
        one, _ = f.CountLines(data, [[4]])
        assert int(one[0]) == int(count[4])
    finally:
        f.close()


def test_finder_term_stats_need_the_device_route():
    f = Finder(GpuEngine.__new__(GpuEngine), PyRegexpEngine(), True)
    try:
        f.AddExpression('"a" and r"b+"')
        for call in (lambda: f.TermStatsLines(b"a bb\n"), lambda: f.TermStatsLines(b"a bb\n", kept=False), lambda: f.CountExpressions(b"a bb\n")):
            with pytest.raises(FinderError) as ei:
                call()
            assert ei.value.code == _lib.GFT_E_UNSUPPORTED
        lowered = C.c_int(0)
        assert _lib.load().gft_finder_term_stats_device(f._h, None, None, 0, None, None, 0, 0, None, None, None,
                                                        C.byref(lowered)) == _lib.GFT_E_UNSUPPORTED
    finally:
        f.close()
