"""The four batch calls over a term list (gft_batch_term_stats_device, gft_batch_top_docs_device and their whole-word twins) through
their shared front end (csrc/gft_term_list.cpp): the 2 x 2 x 2 matrix statistics / top, plain / whole words, without / with a hit
bitmap against the references of term_stats.py and rank.py applied to the list that the corresponding list call returns on its own
(gft_scan_device, gft_hit_spans_device, gft_scan_words_device, gft_hit_spans_words_device); a want mask; the degenerate lists, where
the count-then-fill protocol skips its fill call while the shared buffers hold an older, longer list; the four calls in turn on one
handle; the nonascii return, which writes nothing; the launch counts of every cell; and the finder's calls on a blob that is lowered
on the device against the same blob lowered on the host.  All comparisons are exact."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before libgft.so is loaded: one HIP runtime)

import fold_cases as FC
import rank as RK
import term_stats as TS
from gofindthem_amd import _lib
from gofindthem_amd.engine import Engine, pack
from gofindthem_amd.finder import EmptyRgxEngine, Finder, GpuEngine
from test_gpu_rank import LOG, LOG_EXPRS, TERMS, TEXTS, _download, to_lower

pytestmark = pytest.mark.gpu

U, AND, OR = 1 << 28, 2 << 28, 3 << 28                              # program words: a term, the two connectives
N = len(TEXTS)
K = 20
SENTINEL = 0x5A5A5A5A5A5A5A5A
FOLD = _lib.GFT_FOLD_ASCII
CELLS = [(words, bitmap) for words in (False, True) for bitmap in (False, True)]


def dev(a):
    a = np.ascontiguousarray(a)
    signed = a.view({1: np.uint8, 4: np.int32, 8: np.int64}[a.dtype.itemsize])
    return torch.from_numpy(np.concatenate([signed.ravel(), np.zeros(1, signed.dtype)])).cuda()[:a.size]


def ptr(t):
    return t.data_ptr() if t is not None else None


class Batch:
    """a batch on the device with the rows process_device and process_words_device leave for it"""

    def __init__(self, e, texts, fold=False):
        blob, off = pack(texts)
        self.n = len(texts)
        self.text = torch.from_numpy(np.concatenate([blob, np.zeros(64, np.uint8)])).cuda()
        self.off = dev(off)
        self.bm, self.bm_words = (torch.zeros((self.n, (e.n_exprs + 31) // 32), dtype=torch.int32, device="cuda") for _ in range(2))
        torch.cuda.synchronize()
        e.process_device(self.text.data_ptr(), self.off.data_ptr(), self.n, self.bm.data_ptr(), fold=fold)
        e.process_words_device(self.text.data_ptr(), self.off.data_ptr(), self.n, self.bm_words.data_ptr(), fold=fold)

    def rows(self, words, lo=0, n=None):
        return (self.bm_words if words else self.bm)[lo:lo + (self.n if n is None else n)]


@pytest.fixture(scope="module")
def eng():
    e = Engine()
    e.build(TERMS)
    t = {name: i for i, name in enumerate(e.terms())}
    e.set_programs([[U | t[b"cat"], U | t[b"hat"], AND], [U | t[b"the"]], [U | t[b"zebra"], U | t[b"mat"], OR]])
    yield e
    e.close()


@pytest.fixture(scope="module")
def batch(eng):
    return Batch(eng, TEXTS)


WEIGHTS = np.array([3, 0, 10, 1, 7, 2], np.uint32)
_lists = {}


def the_list(e, B, words, bitmap, lo=0, n=None, want=None, fold=False, rows=None):
    """(off, term) as the cell's list call returns it for documents [lo, lo + n) of the batch (computed once for every key)"""
    n = B.n if n is None else n
    key = (id(B), words, bitmap, lo, n, None if want is None else tuple(want), fold, None if rows is None else id(rows))
    if key not in _lists:
        d_off = B.off[lo:lo + n + 1]
        if bitmap:
            call = e.hit_spans_words_device if words else e.hit_spans_device
            so, _, _, st = call(B.text, d_off, B.rows(words, lo, n) if rows is None else rows, want, fold=fold)[:4]
            _lists[key] = so.cpu().numpy().view(np.uint64), st.cpu().numpy().view(np.uint32)
        else:
            m = (e.scan_words_device if words else e.scan_device)(B.text.data_ptr(), d_off.data_ptr(), n, fold=fold)
            _lists[key] = _download(m, n)
    return _lists[key]


def stats_call(e, B, words, rows, lo=0, n=None, want=None, flags=0, scan_flags=0, doc_base=0, outs=None, nonascii=True):
    """one statistics call -> (occ, docs, first) as uint64 arrays, *nonascii (None when NULL was handed in)"""
    n = B.n if n is None else n
    fn = _lib.load().gft_batch_term_stats_words_device if words else _lib.load().gft_batch_term_stats_device
    outs = outs if outs is not None else [torch.full((e.n_terms,), SENTINEL, dtype=torch.int64, device="cuda") for _ in range(3)]
    again = C.c_int(5)
    w = np.ascontiguousarray(want, dtype=np.uint32) if want is not None else None
    torch.cuda.synchronize()
    assert fn(e._h, B.text.data_ptr(), B.off[lo:].data_ptr(), n, scan_flags, ptr(rows), w.ctypes.data if w is not None else None, flags, doc_base,
              *(o.data_ptr() for o in outs), C.byref(again) if nonascii else None) == 0
    return [o.cpu().numpy().view(np.uint64) for o in outs], (again.value if nonascii else None)


def top_call(e, B, words, rows, lo=0, n=None, want=None, flags=0, scan_flags=0, k=K, weights=WEIGHTS, nonascii=True):
    """one top call -> (scores, top_idx, top_score) as uint64 arrays (the top arrays whole, sentinel behind the list), n_top, *nonascii"""
    n = B.n if n is None else n
    fn = _lib.load().gft_batch_top_docs_words_device if words else _lib.load().gft_batch_top_docs_device
    score = torch.full((max(n, 1),), SENTINEL, dtype=torch.int64, device="cuda")
    ti, ts = (torch.full((k,), SENTINEL, dtype=torch.int64, device="cuda") for _ in range(2))
    n_top, again = C.c_uint64(77), C.c_int(5)
    w = np.ascontiguousarray(want, dtype=np.uint32) if want is not None else None
    torch.cuda.synchronize()
    assert fn(e._h, B.text.data_ptr(), B.off[lo:].data_ptr(), n, scan_flags, ptr(rows), w.ctypes.data if w is not None else None,
              weights.ctypes.data if weights is not None else None, flags, k, RK.BASE, score.data_ptr(), ti.data_ptr(), ts.data_ptr(),
              C.byref(n_top), C.byref(again) if nonascii else None) == 0
    return [t.cpu().numpy().view(np.uint64) for t in (score[:n], ti, ts)], int(n_top.value), (again.value if nonascii else None)


def check_stats(e, B, words, bitmap, lo=0, n=None, want=None, rows=None, lst=None):
    n = B.n if n is None else n
    rows = (B.rows(words, lo, n) if rows is None else rows) if bitmap else None
    off, term = lst if lst is not None else the_list(e, B, words, bitmap, lo, n, want)
    got, again = stats_call(e, B, words, rows, lo, n, want, doc_base=9)
    assert again == 0
    for g, w in zip(got, TS.reference(off, term, n, e.n_terms, 9)):
        assert (g == w).all(), (words, bitmap, lo, n)
    return term.size


def check_top(e, B, words, bitmap, lo=0, n=None, want=None, rows=None, lst=None, flags=0):
    n = B.n if n is None else n
    rows = (B.rows(words, lo, n) if rows is None else rows) if bitmap else None
    off, term = lst if lst is not None else the_list(e, B, words, bitmap, lo, n, want)
    (score, ti, ts), n_top, again = top_call(e, B, words, rows, lo, n, want, flags)
    want_score = RK.score_reference(off, term, n, e.n_terms, WEIGHTS, bool(flags))
    wi, wv = RK.top_reference(want_score, K, RK.BASE)
    assert again == 0 and n_top == wi.size
    assert (score == want_score).all() and (ti[:n_top] == wi).all() and (ts[:n_top] == wv).all(), (words, bitmap, lo, n)
    assert (ti[n_top:] == SENTINEL).all() and (ts[n_top:] == SENTINEL).all()
    return n_top


@pytest.mark.parametrize("words,bitmap", CELLS)
def test_matrix(eng, batch, words, bitmap):
    """every cell on the full batch, and with a want mask that keeps the second expression only"""
    assert check_stats(eng, batch, words, bitmap) and check_top(eng, batch, words, bitmap)
    check_top(eng, batch, words, bitmap, flags=RK.DISTINCT)
    if bitmap:
        one = np.array([2], np.uint32)
        off, term = the_list(eng, batch, words, True, want=one)
        assert 0 < term.size < the_list(eng, batch, words, True)[1].size
        assert check_stats(eng, batch, words, True, want=one) and check_top(eng, batch, words, True, want=one)
    else:
        # (`at` inside `cat`, `hat`, `mat`: the filter drops matches)
        assert the_list(eng, batch, True, False)[1].size < the_list(eng, batch, False, False)[1].size


@pytest.mark.parametrize("words", [False, True])
def test_degenerate_lists(eng, batch, words):
    """the lists that skip the fill call, each behind a full batch's call that left its longer list in the shared buffers"""
    empty = np.zeros(1, np.uint64), np.zeros(0, np.uint32)
    zeros = torch.zeros_like(batch.bm)
    none = np.zeros(1, np.uint32)
    torch.cuda.synchronize()
    for check in (check_stats, check_top):
        for bitmap in (False, True):
            # no documents
            assert check(eng, batch, words, True)
            assert check(eng, batch, words, bitmap, n=0, lst=empty) == 0
        # an all-zero bitmap, a want mask of zeros: a list of N empty rows
        nothing = np.zeros(N + 1, np.uint64), np.zeros(0, np.uint32)
        assert check(eng, batch, words, True)
        assert check(eng, batch, words, True, rows=zeros, lst=nothing) == 0
        assert check(eng, batch, words, True)
        assert check(eng, batch, words, True, want=none, lst=nothing) == 0
        # a run cut from the middle of the blob: d_doc_off[0] != 0
        for bitmap in (False, True):
            assert check(eng, batch, words, True)
            assert check(eng, batch, words, bitmap, lo=6, n=13)
    (occ, docs, first), _ = stats_call(eng, batch, words, zeros)
    assert not occ.any() and not docs.any() and (first == TS.MAX).all()
    (score, _, _), n_top, _ = top_call(eng, batch, words, zeros)
    assert not score.any() and n_top == 0


def test_buffer_reuse(eng, batch):
    """one handle, one kept list: plain statistics of the full batch, whole-word top of seven documents, plain top of the full batch,
    whole-word statistics of the seven"""
    for _ in range(2):
        assert check_stats(eng, batch, False, True)
        assert check_top(eng, batch, True, True, n=7)
        assert check_top(eng, batch, False, True)
        assert check_stats(eng, batch, True, True, n=7)


def test_nonascii_return(eng):
    """a batch that is not fold-safe under GFT_FOLD_ASCII: with nonascii the calls return before anything of theirs is written, the
    verdict published; with NULL they go on and count the ASCII fold's matches"""
    L = _lib.load()
    B = Batch(eng, list(TEXTS[:6]) + [b"the cat " + FC.SENSITIVE["C3 89"] + b" hat"], fold=True)
    for words, bitmap in CELLS:
        rows = B.rows(words) if bitmap else None
        for flags in (0, TS.ACC):
            outs, again = stats_call(eng, B, words, rows, flags=flags, scan_flags=FOLD)
            assert again == 1 and L.gft_last_nonascii(eng._h) == 1 and all((o == SENTINEL).all() for o in outs), (words, bitmap, flags)
        outs, n_top, again = top_call(eng, B, words, rows, scan_flags=FOLD)
        assert again == 1 and L.gft_last_nonascii(eng._h) == 1 and n_top == 0 and all((o == SENTINEL).all() for o in outs), (words, bitmap)
        # NULL: the call goes on
        off, term = the_list(eng, B, words, bitmap, fold=True)
        assert term.size
        outs, _ = stats_call(eng, B, words, rows, scan_flags=FOLD, nonascii=False)
        for g, w in zip(outs, TS.reference(off, term, B.n, eng.n_terms)):
            assert (g == w).all(), (words, bitmap)
        (score, ti, ts), n_top, _ = top_call(eng, B, words, rows, scan_flags=FOLD, nonascii=False)
        want = RK.score_reference(off, term, B.n, eng.n_terms, WEIGHTS)
        wi, wv = RK.top_reference(want, K, RK.BASE)
        assert (score == want).all() and n_top == wi.size and (ti[:n_top] == wi).all() and (ts[:n_top] == wv).all(), (words, bitmap)
        assert L.gft_last_nonascii(eng._h) == 1
    # a batch inside ASCII under the same flag: the calls go on, *nonascii stays 0
    A = Batch(eng, TEXTS[:6], fold=True)
    outs, again = stats_call(eng, A, False, A.rows(False), scan_flags=FOLD)
    assert again == 0 and L.gft_last_nonascii(eng._h) == 0 and not any((o == SENTINEL).all() for o in outs)


CATEGORIES = ("scan", "span_mark", "span_scan", "span_place", "word_check", "word_mark", "word_scan", "word_place", "stats_check", "stats_count",
              "score_check", "score_docs", "top_max", "top_select", "top_place", "top_sort")
# the categories that are not 0, per (call, words, bitmap): recorded on the commit before the front end
_SPANS = {"span_mark": 2, "span_scan": 2, "span_place": 2}          # count, then fill
_FILTER = {"word_check": 1, "word_mark": 1, "word_scan": 1, "word_place": 1}
_SOURCE = {(False, False): {"scan": 1}, (False, True): {"scan": 2, **_SPANS}, (True, False): {"scan": 1, **_FILTER},
           # (the whole-word spans call counts and fills its own input: two plain spans calls for each of its two)
           (True, True): {"scan": 4, **{c: 2 * v for c, v in _SPANS.items()}, **{c: 2 * v for c, v in _FILTER.items()}}}
_CONSUMER = {"stats": {"stats_check": 1, "stats_count": 1},
             "top": {"score_check": 1, "score_docs": 1, "top_select": 1, "top_place": 1, "top_sort": 1}}
LAUNCHES = {(call, words, bitmap): {**_SOURCE[words, bitmap], **_CONSUMER[call]} for call in _CONSUMER for words, bitmap in _SOURCE}


def launches(e, call):
    e.profile(True)
    e.profile_reset()
    try:
        call()
        return {c: e.profile_read(c)[1] for c in CATEGORIES if e.profile_read(c)[1]}
    finally:
        e.profile(False)


def test_launch_counts(eng, batch):
    """the profile's launch counts of every cell on the full batch are those of the commit before the shared front end, which produced
    the table above: no scan and no pass was added or dropped"""
    got = {}
    for words, bitmap in CELLS:
        rows = batch.rows(words) if bitmap else None
        got["stats", words, bitmap] = launches(eng, lambda: stats_call(eng, batch, words, rows))
        got["top", words, bitmap] = launches(eng, lambda: top_call(eng, batch, words, rows))
    for key in sorted(got):
        print("    %r: %r," % (key, got[key]))
    assert got == LAUNCHES


@pytest.mark.parametrize("whole_words", [False, True])
def test_finder_lowered_on_the_device_or_on_the_host(whole_words):
    """TermStatsLines, TopLines and SpansLines of a blob with one line that leaves ASCII in upper case: lowered on the device, with the
    results of the same blob lowered on the host"""
    lines = [ln + b"\n" for ln in LOG]
    lines[3] = "KERNEL: OOM-killer invoked by CAFÉ root PASSWORD password\n".encode()
    data, low_data = b"".join(lines), b"".join(to_lower(ln) for ln in lines)
    assert data != low_data and len(data) == len(low_data)
    f = Finder(GpuEngine.__new__(GpuEngine), EmptyRgxEngine(), False, whole_words=whole_words)
    try:
        for ex, tag in LOG_EXPRS:
            f.AddExpressionWithTag(ex, tag)
        for want in (None, f.want_mask(tags=["alert"])):
            for kept in (True, False):
                if not kept and want is not None:
                    continue
                got, low = f.TermStatsLines(data, want, kept=kept)
                assert low is True and got and (got, False) == f.TermStatsLines(low_data, want, kept=kept)
                got, low = f.TopLines(data, k=7, want=want, kept=kept, weights={"password": 5, None: 2})
                host, host_low = f.TopLines(low_data, k=7, want=want, kept=kept, weights={"password": 5, None: 2})
                assert low is True and host_low is False and got and [g[:2] for g in got] == [h[:2] for h in host]
                assert all(b == lines[d] for d, _, b in got)
            idx, spans, low = f.SpansLines(data, want)
            h_idx, h_spans, h_low = f.SpansLines(low_data, want)
            assert low is True and h_low is False and (idx == h_idx).all() and spans == h_spans and 3 in idx.tolist()
    finally:
        f.close()
