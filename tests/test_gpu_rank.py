"""The ranking calls on the device (csrc/gft_rank.hip): gft_score_docs_device, gft_top_docs_device and gft_gather_docs_device against
the numpy references of rank.py on the cases test_rank_host.py runs through the host walks -- the borders from gft_debug_rank_shape
and gft_debug_select_shape, both score modes, the 64-bit carry, the select's ties at the threshold across tiles, every cap cut of the
gather, the refusals, which leave every output byte for byte and the handle usable, the overlaps --, the calls behind the scan and
the spans, and the finder layer end to end: TopLines against scores counted from SpansLines' own output and from the oracle's match
list, with a batch that is lowered.  All comparisons are exact."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before libgft.so is loaded: one HIP runtime)

import rank as RK
from gofindthem_amd import _lib
from gofindthem_amd.engine import Engine, pack, rank_shape, select_shape
from gofindthem_amd.finder import EmptyRgxEngine, Finder, FinderError, GpuEngine, PyRegexpEngine
from oracle.pyoracle import Oracle, pack_strings

pytestmark = pytest.mark.gpu

SH = rank_shape()
SCORE = RK.score_cases(SH)
TOP = RK.top_cases(SH)
BLOB, OFF = RK.gather_batch(select_shape())
LISTS = RK.gather_lists(OFF.size - 1)
REFUSALS = RK.score_refusals(SH)


@pytest.fixture(scope="module")
def eng():
    e = Engine()
    yield e
    e.close()


def dev(a):
    """a numpy array of bytes or of 32- or 64-bit words on the device (None stays None; an empty one gets a word, so that it has an
    address)"""
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    signed = a.view({1: np.uint8, 4: np.int32, 8: np.int64}[a.dtype.itemsize])
    return torch.from_numpy(np.concatenate([signed.ravel(), np.zeros(1, signed.dtype)])).cuda()[:a.size]


def back(a, t):
    a[:] = t.cpu().numpy().view(a.dtype)


def ptr(t):
    return t.data_ptr() if t is not None else None


def score_runner(e):
    def run(off, term, n_docs, n_terms, weights, flags, score):
        d_off, d_term, d_score = dev(off), dev(term), dev(score)
        mx = C.c_uint64(0)
        w = np.ascontiguousarray(weights, dtype=np.uint32) if weights is not None and len(weights) else None
        torch.cuda.synchronize()
        rc = _lib.load().gft_score_docs_device(e._h, ptr(d_off) if n_docs else None, ptr(d_term), n_docs, n_terms,
                                               w.ctypes.data if w is not None else None, flags, ptr(d_score) if n_docs else None, C.byref(mx))
        torch.cuda.synchronize()
        back(score, d_score)
        return rc, int(mx.value)
    return run


def top_runner(e):
    def run(score, n_docs, k, doc_base, top_idx, top_score):
        d_score, d_ti, d_ts = dev(score), dev(top_idx), dev(top_score)
        n = C.c_uint64(0)
        torch.cuda.synchronize()
        rc = _lib.load().gft_top_docs_device(e._h, ptr(d_score) if n_docs else None, n_docs, k, doc_base, ptr(d_ti), ptr(d_ts), C.byref(n))
        torch.cuda.synchronize()
        back(top_idx, d_ti)
        back(top_score, d_ts)
        return rc, int(n.value)
    return run


def gather_runner(e, d_blob, d_off):
    def run(blob, off, n_docs, idx, idx_base, out, cap, out_off):
        d_idx, d_out, d_oo = dev(idx), dev(out), dev(out_off)
        total = C.c_uint64(0)
        torch.cuda.synchronize()
        rc = _lib.load().gft_gather_docs_device(e._h, d_blob.data_ptr(), d_off.data_ptr(), n_docs, ptr(d_idx) if idx.size else None, idx.size, idx_base,
                                                ptr(d_out), cap, d_oo.data_ptr(), C.byref(total))
        torch.cuda.synchronize()
        if out is not None:
            back(out, d_out)
        back(out_off, d_oo)
        return rc, int(total.value)
    return run


@pytest.fixture(scope="module")
def batch():
    return dev(BLOB), dev(OFF)


def test_symbols_present():
    L = _lib.load()
    for name in ("gft_score_docs_device", "gft_top_docs_device", "gft_gather_docs_device", "gft_batch_top_docs_device",
                 "gft_batch_top_docs_words_device", "gft_finder_top_docs_device", "gft_debug_rank_shape"):
        assert hasattr(L, name) and name in _lib.SYMBOLS


@pytest.mark.parametrize("case", SCORE, ids=[c.name for c in SCORE])
def test_score(eng, case):
    RK.check_score(score_runner(eng), case)


def test_null_weights_are_ones(eng):
    RK.check_null_weights_are_ones(score_runner(eng), SCORE)


@pytest.mark.parametrize("r", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_score_refusals(eng, r):
    RK.check_score_refusal(score_runner(eng), *r[1:])
    RK.check_score(score_runner(eng), SCORE[0])                     # the handle stays usable


@pytest.mark.parametrize("c", TOP, ids=[c[0] for c in TOP])
def test_top(eng, c):
    name, score, ks = c
    for k in ks:
        RK.check_top(top_runner(eng), name, score, k)


def test_top_refusals(eng):
    score = np.arange(1, 9000, dtype=np.uint64)
    ti, ts = np.full(5000, RK.PATTERN, np.uint64), np.full(5000, RK.PATTERN, np.uint64)
    assert top_runner(eng)(score, score.size, SH["max_k"] + 1, 0, ti, ts)[0] == RK.E_INVALID
    assert (ti == RK.PATTERN).all() and (ts == RK.PATTERN).all()
    RK.check_top(top_runner(eng), "after", score, SH["max_k"])


@pytest.mark.parametrize("lst", LISTS, ids=[n for n, _ in LISTS])
def test_gather(eng, batch, lst):
    RK.check_gather(gather_runner(eng, *batch), BLOB, OFF, *lst)


def test_gather_idx_base(eng, batch):
    RK.check_gather(gather_runner(eng, *batch), BLOB, OFF, *LISTS[2], idx_base=(1 << 40) + 1)


def test_gather_refusals(eng, batch):
    RK.check_gather_refusals(gather_runner(eng, *batch), BLOB, OFF)
    RK.check_gather(gather_runner(eng, *batch), BLOB, OFF, *LISTS[2])


def test_overlaps(eng, batch):
    """an output that overlaps an input or the other output: refused, nothing written"""
    L = _lib.load()
    case = next(c for c in SCORE if c.name == "cut_middle")
    n, nt = case.n_docs, case.n_terms
    d_off, d_term = dev(case.off), dev(case.term)
    keep_off, keep_term = d_off.clone(), d_term.clone()
    torch.cuda.synchronize()
    for name, out in (("offsets", d_off.data_ptr() + 8), ("offsets_last_word", d_off.data_ptr() + 8 * n), ("entries", d_term.data_ptr() + 778 * 4)):
        assert L.gft_score_docs_device(eng._h, d_off.data_ptr(), d_term.data_ptr(), n, nt, None, 0, out, None) == RK.E_INVALID, name
        assert torch.equal(d_off, keep_off) and torch.equal(d_term, keep_term), name
    # (the entries in front of off[0] are no input: the scores may lie there)
    assert 2 * n <= 777 and L.gft_score_docs_device(eng._h, d_off.data_ptr(), d_term.data_ptr(), n, nt, None, 0, d_term.data_ptr(), None) == 0
    pool = torch.arange(1, 301, dtype=torch.int64, device="cuda")
    keep = pool.clone()
    p, nn = pool.data_ptr(), C.c_uint64(0)
    torch.cuda.synchronize()
    for name, (ti, ts) in {"idx_scores": (p + 90 * 8, p + 200 * 8), "score_scores": (p + 200 * 8, p + 95 * 8), "idx_score": (p + 800, p + 840)}.items():
        assert L.gft_top_docs_device(eng._h, p, 100, 10, 0, ti, ts, C.byref(nn)) == RK.E_INVALID, name
        assert torch.equal(pool, keep), name
    assert L.gft_top_docs_device(eng._h, p, 100, 10, 0, p + 800, p + 880, C.byref(nn)) == 0 and nn.value == 10
    assert pool[100:110].tolist() == list(range(99, 89, -1)) and pool[110:120].tolist() == list(range(100, 90, -1))
    # the gather's outputs over the text, the offsets, the list and each other
    d_blob, d_doff = (t.clone() for t in batch)
    idx = torch.arange(4, dtype=torch.int64, device="cuda")
    spare, spare_off = torch.zeros(64, dtype=torch.uint8, device="cuda"), torch.zeros(8, dtype=torch.int64, device="cuda")
    lo, tot = int(OFF[0]), C.c_uint64(0)
    sets = {"out_text": (d_blob.data_ptr() + lo + 8, spare_off.data_ptr()), "out_offsets": (d_doff.data_ptr() + 8, spare_off.data_ptr()),
            "out_list": (idx.data_ptr(), spare_off.data_ptr()), "off_text": (spare.data_ptr(), d_blob.data_ptr() + lo + 3),
            "off_offsets": (spare.data_ptr(), d_doff.data_ptr() + 16), "off_list": (spare.data_ptr(), idx.data_ptr()),
            "out_off": (spare_off.data_ptr(), spare_off.data_ptr())}
    torch.cuda.synchronize()
    for name, (out, oo) in sets.items():
        assert L.gft_gather_docs_device(eng._h, d_blob.data_ptr(), d_doff.data_ptr(), OFF.size - 1, idx.data_ptr(), 4, 0, out, 16, oo,
                                        C.byref(tot)) == RK.E_INVALID, name
        assert torch.equal(d_blob, batch[0]) and torch.equal(d_doff, batch[1]) and idx.tolist() == [0, 1, 2, 3], name


def test_engine_wrappers_and_profile_names(eng, batch):
    case = next(c for c in SCORE if c.name == "ranges")
    want = RK.score_reference(case.off, case.term, case.n_docs, case.n_terms, case.weights, True)
    eng.profile(True)
    eng.profile_reset()
    try:
        score, mx = eng.score_docs_device(dev(case.off), dev(case.term), case.n_docs, case.n_terms, case.weights, distinct=True)
        ti, ts = eng.top_docs_device(score, 65, doc_base=9)
        out, out_off = eng.gather_docs_device(batch[0], batch[1], dev(LISTS[1][1]))
        for cat, times in (("score_check", 1), ("score_docs", 1), ("top_max", 1), ("top_select", 1), ("top_place", 1), ("top_sort", 1),
                           ("gather_place", 2), ("gather_scan", 2), ("gather_copy", 1)):
            assert eng.profile_read(cat)[1] == times, cat
    finally:
        eng.profile(False)
    assert (score.cpu().numpy().view(np.uint64) == want).all() and mx == int(want.max())
    wi, wv = RK.top_reference(want, 65, 9)
    assert (ti.cpu().numpy().view(np.uint64) == wi).all() and (ts.cpu().numpy().view(np.uint64) == wv).all()
    w_out, w_off = RK.gather_reference(BLOB, OFF, LISTS[1][1])
    assert (out.cpu().numpy() == w_out).all() and (out_off.cpu().numpy().view(np.uint64) == w_off).all()


U, AND, OR = 1 << 28, 2 << 28, 3 << 28                              # program words: a term, the two connectives
TEXTS = [b"the cat sat on the mat with the hat", b"", b"a cat, a hat and a bat", b"no match here", b"the the the the", b"hat" * 50] * 30
TERMS = [b"the", b"cat", b"hat", b"at", b"mat", b"zebra"]


def batch_top(e, fn, text, d_off, n, bitmap, weights, flags, k, want_scores=True):
    score = torch.full((n,), 0x11, dtype=torch.int64, device="cuda") if want_scores else None
    ti, ts = (torch.full((k,), -7, dtype=torch.int64, device="cuda") for _ in range(2))
    n_top, again = C.c_uint64(0), C.c_int(5)
    w = np.ascontiguousarray(weights, dtype=np.uint32) if weights is not None else None
    torch.cuda.synchronize()
    assert fn(e._h, text.data_ptr(), d_off.data_ptr(), n, 0, ptr(bitmap), None, w.ctypes.data if w is not None else None, flags, k, RK.BASE,
              ptr(score), ti.data_ptr(), ts.data_ptr(), C.byref(n_top), C.byref(again)) == 0 and again.value == 0
    m = int(n_top.value)
    assert bool((ti[m:] == -7).all()) and bool((ts[m:] == -7).all())
    return (score.cpu().numpy().view(np.uint64) if want_scores else None), ti[:m].cpu().numpy().view(np.uint64), ts[:m].cpu().numpy().view(np.uint64)


def test_behind_the_scan(eng):
    """gft_batch_top_docs_device against the reference applied to gft_scan_device's own list and to gft_hit_spans_device's; the
    words twin against the filtered list"""
    L = _lib.load()
    eng.build(TERMS)
    t = {name: i for i, name in enumerate(eng.terms())}
    eng.set_programs([[U | t[b"cat"], U | t[b"hat"], AND], [U | t[b"the"]], [U | t[b"zebra"], U | t[b"mat"], OR]])
    blob, off = pack(TEXTS)
    n = len(TEXTS)
    text = torch.from_numpy(np.concatenate([blob, np.zeros(64, np.uint8)])).cuda()
    d_off = dev(off)
    weights = np.array([3, 0, 10, 1, 7, 2][:eng.n_terms], np.uint32)
    torch.cuda.synchronize()
    mo, ti_, _ = eng.scan(blob, off)
    for w, flags, k in ((None, 0, 10), (weights, 0, 4096), (weights, RK.DISTINCT, 7)):
        want = RK.score_reference(mo, ti_, n, eng.n_terms, w, bool(flags))
        for want_scores in (True, False):
            score, gi, gv = batch_top(eng, L.gft_batch_top_docs_device, text, d_off, n, None, w, flags, k, want_scores)
            wi, wv = RK.top_reference(want, k, RK.BASE)
            assert (score is None or (score == want).all()) and (gi == wi).all() and (gv == wv).all() and gi.size
    # the kept matches: the spans' list
    bm = torch.zeros((n, (eng.n_exprs + 31) // 32), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng.process_device(text.data_ptr(), d_off.data_ptr(), n, bm.data_ptr())
    span_off, _, _, span_term = eng.hit_spans_device(text, d_off, bm)[:4]
    want = RK.score_reference(span_off.cpu().numpy().view(np.uint64), span_term.cpu().numpy().view(np.uint32), n, eng.n_terms, weights, False)
    score, gi, gv = batch_top(eng, L.gft_batch_top_docs_device, text, d_off, n, bm, weights, 0, 20)
    wi, wv = RK.top_reference(want, 20, RK.BASE)
    assert (score == want).all() and (gi == wi).all() and (gv == wv).all() and gi.size
    # the words twin: the scan's list filtered at word borders
    m = eng.scan_words_device(text.data_ptr(), d_off.data_ptr(), n)
    w_off, w_term = _download(m, n)
    assert 0 < w_term.size < ti_.size                               # (`at` inside `cat`, `hat`, `mat`: the filter drops matches)
    want = RK.score_reference(w_off, w_term, n, eng.n_terms, weights, True)
    score, gi, gv = batch_top(eng, L.gft_batch_top_docs_words_device, text, d_off, n, None, weights, RK.DISTINCT, 20)
    wi, wv = RK.top_reference(want, 20, RK.BASE)
    assert (score == want).all() and (gi == wi).all() and (gv == wv).all() and gi.size


def _download(m, n_docs):
    """(match_off, term_id) of a GftMatches with device pointers, as numpy arrays"""
    hip = C.CDLL("libamdhip64.so")

    def get(p, n, dt):
        a = np.zeros(max(n, 1), dtype=dt)
        if n:
            assert hip.hipMemcpy(C.c_void_p(a.ctypes.data), C.c_void_p(p), C.c_size_t(a.itemsize * n), C.c_int(2)) == 0
        return a[:n]
    return get(m.match_off, n_docs + 1, np.uint64), get(m.term_id, int(m.n_matches), np.uint32)


LOG = [b"GET /index.html 200", b"POST /login 401 bad password for root", b"GET /admin 403", b"kernel: oom-killer invoked", b"",
       b"POST /login 200 root", b"GET /health 200", b"sshd: Failed password for root from 10.0.0.7", b"cron: job done password password"] * 5
LOG_EXPRS = [('"password" and "root"', "auth"), ('"403" or "oom"', "alert"), ('"GET" and not "200"', "alert"), ('inord("POST" and "login")', "auth"),
             ('"cron"', "")]


def log_finder(**kw):
    f = Finder(GpuEngine.__new__(GpuEngine), EmptyRgxEngine(), False, **kw)
    for e, t in LOG_EXPRS:
        f.AddExpressionWithTag(e, t)
    return f


def to_lower(b):
    out = np.zeros(3 * len(b) + 1, dtype=np.uint8)
    n = C.c_uint64(0)
    assert _lib.load().gft_to_lower(b, len(b), out.ctypes.data, out.size, C.byref(n)) == 0
    return out[:n.value].tobytes()


def expected_lines(scores, lines, k):
    """the contract over a {line: score} dict"""
    order = sorted((d for d, s in scores.items() if s > 0), key=lambda d: (-scores[d], d))[:k]
    return [(d, scores[d], lines[d]) for d in order]


@pytest.mark.parametrize("lowered", [False, True])
@pytest.mark.parametrize("whole_words", [False, True])
def test_finder_top_lines(lowered, whole_words):
    lines = [ln + b"\n" for ln in LOG]
    if lowered:
        lines[3] = "KERNEL: OOM-killer invoked by CAFÉ root PASSWORD password\n".encode()
    data = b"".join(lines)
    f = log_finder(whole_words=whole_words)
    try:
        weights = {"password": 5, "oom": 100, None: 2}
        for want in (None, f.want_mask(tags=["alert"])):
            idx, spans, low = f.SpansLines(data, want)
            per_line = {d: [s[2] for s in sp] for d, sp in zip(idx.tolist(), spans)}
            wt = lambda t: weights.get(t.decode(), weights[None])   # noqa: E731
            variants = (({}, lambda ts: len(ts)), ({"weights": weights}, lambda ts: sum(wt(t) for t in ts)),
                        ({"distinct": True}, lambda ts: len(set(ts))), ({"weights": weights, "distinct": True}, lambda ts: sum(wt(t) for t in set(ts))))
            for kw, fn in variants:
                for k in (3, 100):
                    got, low2 = f.TopLines(data, k=k, want=want, **kw)
                    assert low == low2 == lowered
                    assert got == expected_lines({d: fn(ts) for d, ts in per_line.items()}, lines, k) and got, (kw, k)
        # every dictionary match: the oracle's list over the text the finder scans
        if not whole_words:
            kw = sorted(k.encode() for k in f.GetKeywords())
            orc = Oracle(kw)
            blob, off = pack_strings([to_lower(ln) for ln in lines])
            mo, ti, _ = orc.scan(blob, off, fold=False)
            sc = RK.score_reference(mo, ti, len(lines), orc.n_terms)
            got, low = f.TopLines(data, k=4, kept=False)
            assert got == expected_lines(dict(enumerate(sc.tolist())), lines, 4) and low == lowered
        # the lines are the caller's bytes, the lowered batch's upper-case line among them
        got, low = f.TopLines(data, k=len(lines), weights={"oom": 1000})
        assert got[0][2] == lines[3] and got[0][0] == 3 and all(lines[d] == b for d, _, b in got)
        with pytest.raises(ValueError):
            f.TopLines(data, weights={"nosuchword": 1})
        assert f.TopLines(b"", k=3) == ([], False)
    finally:
        f.close()


def test_finder_top_device_scores(eng):
    """TopDevice hands every line's score back; a weight of 0 for every keyword lists nothing"""
    data = b"".join(ln + b"\n" for ln in LOG)
    f = log_finder()
    try:
        buf = f._resident(data)
        off, bm = f.ProcessLinesDevice(buf, len(data))
        idx, val, scores, low = f.TopDevice(buf, off, bm, k=5)
        sc = scores.cpu().numpy().view(np.uint64)
        wi, wv = RK.top_reference(sc, 5)
        assert (idx.cpu().numpy().view(np.uint64) == wi).all() and (val.cpu().numpy().view(np.uint64) == wv).all() and not low and sc.any()
        nt = int(_lib.load().gft_n_terms(f.engine_handle()))
        idx, val, scores, _ = f.TopDevice(buf, off, bm, k=5, weights=np.zeros(nt, np.uint32))
        assert idx.numel() == 0 and not scores.any()
    finally:
        f.close()


def test_finder_top_needs_the_device_route():
    f = Finder(GpuEngine.__new__(GpuEngine), PyRegexpEngine(), True)
    try:
        f.AddExpression('"a" and r"b+"')
        for call in (lambda: f.TopLines(b"a bb\n"), lambda: f.TopLines(b"a bb\n", kept=False)):
            with pytest.raises(FinderError) as ei:
                call()
            assert ei.value.code == _lib.GFT_E_UNSUPPORTED
        lowered, n_top = C.c_int(0), C.c_uint64(0)
        assert _lib.load().gft_finder_top_docs_device(f._h, None, None, 0, None, None, None, 0, 0, 0, None, None, None, C.byref(n_top),
                                                      C.byref(lowered)) == _lib.GFT_E_UNSUPPORTED
    finally:
        f.close()
