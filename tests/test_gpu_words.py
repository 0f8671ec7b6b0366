"""Whole-word matching on the device (csrc/gft_words.hip): gft_filter_word_matches_device against the Python reference of
word_cases.py on the cases test_words_host.py runs through the host walk -- every neighbour kind on both sides of an occurrence,
the document's borders with letters just outside them, runes cut by a border, every start alignment, the tile's borders from
gft_debug_words_shape, both length sources, positions of last bytes, the cap protocol, the refusals, which leave every output byte
and the handle usable, the overlaps, a seeded random batch --; gft_scan_words_device and gft_process_words_device under every scan
kernel against expressions evaluated in Python over the kept occurrences; the finder with whole_words=True end to end.  All
comparisons are exact."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before libgft.so is loaded: one HIP runtime)

import word_cases as W
from gofindthem_amd import _lib
from gofindthem_amd.engine import Engine, GftError, words_shape
from gofindthem_amd.finder import EmptyRgxEngine, Finder, FinderError, GpuEngine, PyRegexpEngine

pytestmark = pytest.mark.gpu

SH = words_shape()
T = SH["tile_entries"]
NEIGHBOURS = W.neighbour_cases()
BORDERS = W.border_cases(T)
RANDOM = W.random_case()
KERNELS = ["scan5", "scan3", "dfa"]
G32, G64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5
U, AND, OR, NOT, INORD, F = 1 << 28, 2 << 28, 3 << 28, 4 << 28, 5 << 28, 1 << 27


@pytest.fixture(scope="module")
def eng():
    e = Engine()
    yield e
    e.close()


def dev(a):
    """a numpy array on the device (None stays None; an empty one gets a word, so that it has an address)"""
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    signed = a.view({1: np.uint8, 4: np.int32, 8: np.int64}[a.dtype.itemsize])
    return torch.from_numpy(np.concatenate([signed.ravel(), np.zeros(1, signed.dtype)])).cuda()[:a.size]


def ptr(t):
    return t.data_ptr() if t is not None else None


def device_filter(e, case, from_terms=True, cap=None, guard=0, with_len=True, with_term=True, at=0):
    """gft_filter_word_matches_device over a case, the text `at` bytes into its allocation -> what word_cases.check_outputs takes"""
    L = _lib.load()
    text = torch.cat([torch.full((at,), ord("a"), dtype=torch.uint8), torch.from_numpy(case.blob)]).cuda()[at:]
    d_doc_off, d_off, d_pos, d_len, d_term, d_tl = (dev(a) for a in (case.doc_off, case.off, case.pos, case.length, case.term, case.term_len))
    args = (e._h, text.data_ptr(), d_doc_off.data_ptr(), case.n_docs, d_off.data_ptr(), ptr(d_pos), None if from_terms else ptr(d_len), ptr(d_term),
            ptr(d_tl) if from_terms else None, len(case.terms) if from_terms else 0, 1 if case.pos_end else 0)
    total = C.c_uint64(0)
    torch.cuda.synchronize()
    if cap is None:
        assert L.gft_filter_word_matches_device(*args, None, None, None, None, 0, C.byref(total)) == 0, e._L.gft_last_error(e._h)
        cap = int(total.value)
    out_off = dev(np.full(case.n_docs + 1 + guard, G64, np.uint64))
    outs = [dev(np.full(cap + guard, G32, np.uint32)) for _ in range(3)]
    use = [True, with_len, with_term]
    rc = L.gft_filter_word_matches_device(*args, out_off.data_ptr(), *(ptr(o) if u and (cap or guard) else None for o, u in zip(outs, use)), cap,
                                          C.byref(total))
    assert rc == 0, e._L.gft_last_error(e._h)
    torch.cuda.synchronize()
    back = [o.cpu().numpy().view(np.uint32) if u else None for o, u in zip(outs, use)]
    return (int(total.value), out_off.cpu().numpy().view(np.uint64)) + tuple(back)


def test_symbols_present():
    L = _lib.load()
    for name in ("gft_filter_word_matches_device", "gft_scan_words_device", "gft_process_words_device", "gft_process_words",
                 "gft_hit_spans_words_device", "gft_finder_set_whole_words", "gft_debug_words_shape"):
        assert hasattr(L, name) and name in _lib.SYMBOLS


@pytest.mark.parametrize("case", NEIGHBOURS + BORDERS, ids=[c.name for c in NEIGHBOURS + BORDERS])
def test_cases(eng, case):
    for from_terms in (True, False):
        W.check_outputs(case, *device_filter(eng, case, from_terms, guard=3), guard=3)


def test_text_at_every_residue(eng):
    case = next(c for c in BORDERS if c.name == "cut_rune")
    for at in range(16):
        W.check_outputs(case, *device_filter(eng, case, True, at=at))


def test_random_batch(eng):
    kept = sum(RANDOM.keep)
    assert kept > 500 and RANDOM.n - kept > 500                    # both outcomes are exercised
    for from_terms in (True, False):
        W.check_outputs(RANDOM, *device_filter(eng, RANDOM, from_terms, guard=2), guard=2)
    # the tensor wrapper: counts, then fills
    d = [dev(a) for a in (RANDOM.blob, RANDOM.doc_off, RANDOM.off, RANDOM.pos, RANDOM.term, RANDOM.term_len)]
    oo, p, ln, tm = eng.filter_word_matches_device(d[0], d[1], d[2], d[3], None, d[4], d[5])
    w_off, w_pos, w_len, w_term = RANDOM.reference()
    assert (oo.cpu().numpy().view(np.uint64) == w_off).all() and (p.cpu().numpy().view(np.uint32) == w_pos).all()
    assert (ln.cpu().numpy().view(np.uint32) == w_len).all() and (tm.cpu().numpy().view(np.uint32) == w_term).all()


@pytest.mark.parametrize("name", ["sentence", "tile_%d" % (T + 1), "pos_end"])
def test_cap_protocol(eng, name):
    case = next(c for c in BORDERS if c.name == name)
    total = sum(case.keep)
    for cap in (0, 1, total - 1, total, total + 5):
        W.check_outputs(case, *device_filter(eng, case, True, cap=cap, guard=4), cap=cap, guard=4)
    for wl, wt in ((False, True), (True, False), (False, False)):
        W.check_outputs(case, *device_filter(eng, case, True, with_len=wl, with_term=wt, guard=1), guard=1)


def test_profile_names(eng):
    case = BORDERS[0]
    eng.profile(True)
    eng.profile_reset()
    try:
        device_filter(eng, case, cap=sum(case.keep))
        for name in ("word_check", "word_mark", "word_scan", "word_place"):
            assert eng.profile_read(name)[1] == 1, name
    finally:
        eng.profile(False)


def broken(name):
    import copy
    c = copy.deepcopy(next(c for c in BORDERS if c.name == "straddle"))
    flags = 0
    if name == "descending_offset":
        c.off[2] = c.off[1] - 1
    elif name == "term_out_of_range":
        c.term[c.n - 1] = len(c.terms)
    elif name == "entry_past_document":
        c.pos[T - 4] = len(c.docs[0]) - 1
    elif name == "entry_before_document":
        flags, c.pos[0] = 1, 0
    elif name == "unknown_flags":
        flags = 4
    return c, flags


@pytest.mark.parametrize("name", ["descending_offset", "term_out_of_range", "entry_past_document", "entry_before_document", "unknown_flags"])
def test_refusals_leave_outputs_and_handle(eng, name):
    L = _lib.load()
    c, flags = broken(name)
    text, d_doc_off, d_off, d_pos, d_term, d_tl = (dev(a) for a in (c.blob, c.doc_off, c.off, c.pos, c.term, c.term_len))
    out_off = dev(np.full(c.n_docs + 1, G64, np.uint64))
    outs = [dev(np.full(c.n, G32, np.uint32)) for _ in range(3)]
    total = C.c_uint64(77)
    torch.cuda.synchronize()
    rc = L.gft_filter_word_matches_device(eng._h, text.data_ptr(), d_doc_off.data_ptr(), c.n_docs, d_off.data_ptr(), d_pos.data_ptr(), None,
                                          d_term.data_ptr(), d_tl.data_ptr(), len(c.terms), flags, out_off.data_ptr(), *(o.data_ptr() for o in outs),
                                          c.n, C.byref(total))
    torch.cuda.synchronize()
    assert rc == W.E_INVALID and total.value == 0
    assert (out_off.cpu().numpy().view(np.uint64) == G64).all() and all((o.cpu().numpy().view(np.uint32) == G32).all() for o in outs)
    W.check_outputs(BORDERS[0], *device_filter(eng, BORDERS[0]))   # the handle stays usable


def test_overlaps(eng):
    L = _lib.load()
    c = next(c for c in BORDERS if c.name == "tile_%d" % T)
    text, d_doc_off, d_off, d_pos, d_term, d_tl = (dev(a) for a in (c.blob, c.doc_off, c.off, c.pos, c.term, c.term_len))
    pool = torch.full((4 * c.n,), 0x77, dtype=torch.int32, device="cuda")
    p = pool.data_ptr()
    sets = {"pos_over_pos": (None, d_pos.data_ptr(), None, None), "len_over_term": (None, p, d_term.data_ptr(), None),
            "pos_and_len": (None, p, p + 4 * 7, None), "off_over_pos": (d_pos.data_ptr(), p, None, None),
            "pos_over_text": (None, (text.data_ptr() + 3) // 4 * 4, None, None), "term_over_offsets": (None, p, None, d_off.data_ptr())}
    keep = [t.clone() for t in (text, d_off, d_pos, d_term)]
    for name, (oo, a, b, t) in sets.items():
        torch.cuda.synchronize()
        rc = L.gft_filter_word_matches_device(eng._h, text.data_ptr(), d_doc_off.data_ptr(), c.n_docs, d_off.data_ptr(), d_pos.data_ptr(), None,
                                              d_term.data_ptr(), d_tl.data_ptr(), len(c.terms), 0, oo, a, b, t, 8, None)
        assert rc == W.E_INVALID, name
        assert bool((pool == 0x77).all()) and all(torch.equal(x, y) for x, y in zip((text, d_off, d_pos, d_term), keep)), name


# ---- gft_scan_words_device / gft_process_words_device ------------------------------------------------------------------------------
TERMS = sorted([b"he", b"she", b"hers", b"na", b"c++", b"a", b"b", b"cat"])      # (the dictionary's order: term ids are indices of this)
HE, SHE, HERS, NA, CPP, A, B_, CAT = (TERMS.index(t) for t in (b"he", b"she", b"hers", b"na", b"c++", b"a", b"b", b"cat"))
PROGRAMS = [[U | HE], [U | SHE, U | HERS, AND], [U | NA, U | CPP, OR], [U | HE, NOT], [U | A | F, U | B_ | F, AND | F, INORD],
            [U | CAT], [U | SHE, U | HE, NOT, AND], [U | B_ | F, U | A | F, AND | F, INORD]]
DOCS = [W.SENTENCE, b"ushers", b"he", b"", b"xa b a", b"a b xa", b"a xb", b"she hers", b"sheds hers", b"c++x na\xc3\xafve", b"na\xc3\xafve",
        b"concatenate", b"cat, dog", b"b_a a-b", b"\xc3he \xc3", b"he\xa9"]


def expected_rows(docs, whole, fold=False):
    """the rows of PROGRAMS over docs, evaluated here from the occurrences (whole: the kept ones alone)"""
    rows = np.zeros((len(docs), 1), dtype=np.uint32)
    for d, doc in enumerate(docs):
        scanned = doc.lower() if fold else doc
        pos = {t: [s for s in W.occurrences(scanned, term) if not whole or W.kept(doc, s, s + len(term))] for t, term in enumerate(TERMS)}
        has = lambda t: bool(pos[t])                                # noqa: E731
        before = lambda x, y: bool(pos[x]) and any(q > pos[x][0] for q in pos[y])   # noqa: E731  INORD(x and y)
        vals = [has(HE), has(SHE) and has(HERS), has(NA) or has(CPP), not has(HE), before(A, B_), has(CAT), has(SHE) and not has(HE), before(B_, A)]
        for i, v in enumerate(vals):
            rows[d, 0] |= np.uint32(int(v) << i)
    return rows


class Resident:
    def __init__(self, docs, lead=b"ab", slack=b"cd"):
        blob = lead + b"".join(docs) + slack + b"a" * 64
        self.text = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
        off = np.zeros(len(docs) + 1, dtype=np.int64)
        off[0] = len(lead)
        off[1:] = len(lead) + np.cumsum([len(d) for d in docs])
        self.off = torch.from_numpy(off).cuda()
        self.n = len(docs)

    def rows(self, words=1):
        return torch.full((self.n, words), 0x5A5A5A5A, dtype=torch.int32, device="cuda")


def make_engine(pos_end=False):
    e = Engine()
    e.build(TERMS, pos_end=pos_end)
    assert e.terms() == TERMS
    e.set_programs(PROGRAMS)
    return e


@pytest.mark.parametrize("pos_end", [False, True], ids=["pos_start", "pos_end"])
@pytest.mark.parametrize("kernel", KERNELS)
def test_scan_and_process_words_under_every_scan_kernel(kernel, pos_end, monkeypatch):
    monkeypatch.setenv("GFT_SCAN_KERNEL", kernel)                   # (read by gft_build)
    e = make_engine(pos_end)
    try:
        r = Resident(DOCS)
        torch.cuda.synchronize()
        # the kept matches: the scan's own list, filtered here
        m = e.scan_device(r.text.data_ptr(), r.off.data_ptr(), r.n)
        nm = int(m.n_matches)
        plain = _download(m, r.n)
        m2 = e.scan_words_device(r.text.data_ptr(), r.off.data_ptr(), r.n)
        words = _download(m2, r.n)
        want_off, want_t, want_p = [0], [], []
        for d in range(r.n):
            for k in range(plain[0][d], plain[0][d + 1]):
                t, p = plain[1][k], plain[2][k]
                s = p + 1 - len(TERMS[t]) if pos_end else p
                if W.kept(DOCS[d], s, s + len(TERMS[t])):
                    want_t.append(t)
                    want_p.append(p)
            want_off.append(len(want_t))
        assert nm == len(plain[1]) and 0 < len(want_t) < nm
        assert (words[0].tolist(), words[1].tolist(), words[2].tolist()) == (want_off, want_t, want_p)
        # the sentence's table
        got = {}
        for k in range(want_off[0], want_off[1]):
            got.setdefault(TERMS[want_t[k]], []).append(want_p[k] + 1 - len(TERMS[want_t[k]]) if pos_end else want_p[k])
        assert got == W.SENTENCE_KEPT
        # the rows: plain before, words, plain after
        want_plain, want_words = expected_rows(DOCS, False), expected_rows(DOCS, True)
        assert (want_plain != want_words).any()
        flip = DOCS.index(b"xa b a")
        assert want_plain[flip, 0] >> 4 & 1 and not want_words[flip, 0] >> 4 & 1      # the INORD whose answer flips
        for whole in (False, True, False, True, True, False):
            bm = r.rows()
            torch.cuda.synchronize()
            if whole:
                e.process_words_device(r.text.data_ptr(), r.off.data_ptr(), r.n, bm.data_ptr())
            else:
                e.process_device(r.text.data_ptr(), r.off.data_ptr(), r.n, bm.data_ptr())
            torch.cuda.synchronize()
            assert (bm.cpu().numpy().view(np.uint32) == (want_words if whole else want_plain)).all(), whole
        # the host-buffer form
        blob = np.frombuffer(b"".join(DOCS) + b"a" * 64, dtype=np.uint8)
        off = np.zeros(len(DOCS) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(d) for d in DOCS])
        assert (e.process_words(blob, off) == want_words).all() and (e.process(blob, off) == want_plain).all()
        # gft_process_again finds no scan of a words call to reuse
        bm = np.zeros((len(DOCS), 1), np.uint32)
        assert _lib.load().gft_process_again(e._h, len(DOCS), None, bm.ctypes.data) == 0
        e.process_words(blob, off)
        assert _lib.load().gft_process_again(e._h, len(DOCS), None, bm.ctypes.data) == W.E_INVALID
        assert _lib.load().gft_scan_kernel(e._h).decode() in (kernel, "scan5", "scan3")
    finally:
        e.close()


def _download(m, n_docs):
    """(match_off, term_id, pos) of a GftMatches with device pointers, as numpy arrays"""
    hip = C.CDLL("libamdhip64.so")

    def get(p, n, dt):
        a = np.zeros(max(n, 1), dtype=dt)
        if n:
            assert hip.hipMemcpy(C.c_void_p(a.ctypes.data), C.c_void_p(p), C.c_size_t(a.itemsize * n), C.c_int(2)) == 0
        return a[:n]
    nm = int(m.n_matches)
    return get(m.match_off, n_docs + 1, np.uint64), get(m.term_id, nm, np.uint32), get(m.pos, nm, np.uint32)


def test_fold_and_flags():
    e = make_engine()
    try:
        docs = [b"Cat CATs cat", b"CATs", b"HE said", b"sHe HERS", b"A B", b"xA B a"]
        r = Resident(docs)
        want = expected_rows(docs, True, fold=True)
        assert want[0, 0] >> 5 & 1 and not want[1, 0] >> 5 & 1 and want[4, 0] >> 4 & 1 and not want[5, 0] >> 4 & 1
        bm = r.rows()
        torch.cuda.synchronize()
        e.process_words_device(r.text.data_ptr(), r.off.data_ptr(), r.n, bm.data_ptr(), fold=True)
        assert (bm.cpu().numpy().view(np.uint32) == want).all()
        assert _lib.load().gft_last_nonascii(e._h) == 0
        m = _download(e.scan_words_device(r.text.data_ptr(), r.off.data_ptr(), r.n, fold=True), r.n)
        cat = [(d, int(p)) for d in range(r.n) for t, p in zip(m[1][m[0][d]:m[0][d + 1]], m[2][m[0][d]:m[0][d + 1]]) if t == CAT]
        assert cat == [(0, 0), (0, 9)]
        # without the fold only the lower-case keyword is there to be kept
        e.process_words_device(r.text.data_ptr(), r.off.data_ptr(), r.n, bm.data_ptr())
        assert (bm.cpu().numpy().view(np.uint32) == expected_rows(docs, True)).all()
        # GFT_SCAN_UNIQUE and GFT_POS_RUNES, any unknown bit
        L = _lib.load()
        mm = _lib.GftMatches()
        for flags in (_lib.GFT_SCAN_UNIQUE, _lib.GFT_POS_RUNES, 8):
            assert L.gft_scan_words_device(e._h, r.text.data_ptr(), r.off.data_ptr(), r.n, flags, C.byref(mm)) == W.E_INVALID
            assert L.gft_process_words_device(e._h, r.text.data_ptr(), r.off.data_ptr(), r.n, flags, bm.data_ptr()) == W.E_INVALID
        # an empty batch
        e.process_words_device(r.text.data_ptr(), r.off.data_ptr(), 0, None)
        assert int(e.scan_words_device(r.text.data_ptr(), r.off.data_ptr(), 0).n_matches) == 0
    finally:
        e.close()


def test_host_solved_expressions_are_refused():
    """an expression beyond the device solver's limits (gft_n_host_exprs > 0): gft_process_words* answer GFT_E_UNSUPPORTED -- the host
    solver is not fed from the kept list --, gft_process_device on the same handle goes on answering"""
    e = Engine()
    try:
        e.build(TERMS)
        side = lambda t: [U | t | F] + [w for _ in range(4499) for w in (U | t | F, OR | F)]   # noqa: E731
        huge = side(A) + side(B_) + [AND | F, INORD]
        e.set_programs([[U | HE], huge])
        assert _lib.load().gft_n_host_exprs(e._h) == 1
        r = Resident([b"he a b", b"ushers b a"])
        bm = r.rows()
        torch.cuda.synchronize()
        with pytest.raises(GftError) as ei:
            e.process_words_device(r.text.data_ptr(), r.off.data_ptr(), r.n, bm.data_ptr())
        assert ei.value.code == W.E_UNSUPPORTED and "gft_n_host_exprs" in str(ei.value)
        assert (bm.cpu().numpy().view(np.uint32) == 0x5A5A5A5A).all()
        e.process_device(r.text.data_ptr(), r.off.data_ptr(), r.n, bm.data_ptr())
        assert bm.cpu().numpy().view(np.uint32).ravel().tolist() == [3, 1]
        # the list itself needs no programs
        assert int(e.scan_words_device(r.text.data_ptr(), r.off.data_ptr(), r.n).n_matches) == 5
    finally:
        e.close()


def test_several_devices_are_refused():
    e = Engine(devices=[0, 0])
    try:
        e.build(TERMS)
        e.set_programs(PROGRAMS)
        r = Resident(DOCS[:3])
        bm = r.rows()
        L = _lib.load()
        mm = _lib.GftMatches()
        torch.cuda.synchronize()
        assert L.gft_process_words_device(e._h, r.text.data_ptr(), r.off.data_ptr(), r.n, 0, bm.data_ptr()) == W.E_UNSUPPORTED
        assert L.gft_scan_words_device(e._h, r.text.data_ptr(), r.off.data_ptr(), r.n, 0, C.byref(mm)) == W.E_UNSUPPORTED
        assert L.gft_filter_word_matches_device(e._h, r.text.data_ptr(), r.off.data_ptr(), 0, None, None, None, None, None, 0, 0, None, None, None,
                                                None, 0, None) == W.E_UNSUPPORTED
    finally:
        e.close()


# ---- the finder ------------------------------------------------------------------------------------------------------------------
LINES = [b"ushers he she hers\n", b"the usher\n", "naïve na “he” he—she\n".encode(), b"c++x c++ x\n", b"concatenate cat\n", b"\n",
         b"HE and She\n", b"asp.net .net\n", b"a_b a b\n"]
EXPRS = ['"he"', '"she" and "hers"', '"na"', '"c++"', '"cat"', '".net"', 'inord("a" and "b")', 'not "he"']
KEYWORDS = [b"he", b"she", b"hers", b"na", b"c++", b"cat", b".net", b"a", b"b"]


def finder_reference(lines, whole, scanned=None):
    """rows, spans and term statistics of EXPRS over the lines from the occurrences found here; scanned: the text the finder scans
    (the lines' lower-case form), on which the borders are judged as well"""
    scanned = scanned or [ln.lower() for ln in lines]
    rows, spans, stats = np.zeros((len(lines), 1), dtype=np.uint32), [], {}
    for d, doc in enumerate(scanned):
        occ = {k: [s for s in W.occurrences(doc, k) if not whole or W.kept(doc, s, s + len(k))] for k in KEYWORDS}
        has = lambda k: bool(occ[k])                                # noqa: E731
        vals = [has(b"he"), has(b"she") and has(b"hers"), has(b"na"), has(b"c++"), has(b"cat"), has(b".net"),
                has(b"a") and any(q > occ[b"a"][0] for q in occ[b"b"]), not has(b"he")]
        wit = [[b"he"], [b"she", b"hers"], [b"na"], [b"c++"], [b"cat"], [b".net"], [b"a", b"b"], []]
        live = {k for v, ks in zip(vals, wit) if v for k in ks}
        for i, v in enumerate(vals):
            rows[d, 0] |= np.uint32(int(v) << i)
        here = sorted((s, -len(k), k) for k in live for s in occ[k])
        spans.append([(s, s + len(k), k) for s, _, k in here])
        for k in live:
            if occ[k]:
                o, n, f = stats.get(k, (0, 0, d))
                stats[k] = (o + len(occ[k]), n + 1, f)
    return rows, spans, stats


def new_finder(whole, case_sensitive=False):
    f = Finder(GpuEngine.__new__(GpuEngine), EmptyRgxEngine(), case_sensitive, whole_words=whole)
    f.AddExpressions(EXPRS)
    return f


@pytest.mark.parametrize("whole", [True, False], ids=["whole_words", "substrings"])
def test_finder_against_the_reference(whole):
    f = new_finder(whole)
    try:
        assert f.whole_words == whole
        data = b"".join(LINES)
        rows, spans, stats = finder_reference(LINES, whole)
        if whole:
            assert (rows != finder_reference(LINES, False)[0]).any()
        assert (f.ProcessTexts(LINES) == rows).all()
        ro, ei, _ = f.ProcessTextsSparse(LINES)
        assert [ei[ro[d]:ro[d + 1]].tolist() for d in range(len(LINES))] == [[i for i in range(len(EXPRS)) if rows[d, 0] >> i & 1] for d in range(len(LINES))]
        assert [r.ExpresionIndex for r in f.ProcessText(LINES[0].decode())] == [i for i in range(len(EXPRS)) if rows[0, 0] >> i & 1]
        off, bm = f.ProcessLines(data)
        assert (bm == rows).all()
        w = f.want_mask([0, 1, 2, 3, 4, 5, 6])
        out, out_off, idx = f.SelectLines(data, w)
        hit = [d for d in range(len(LINES)) if rows[d, 0] & 0x7F]
        assert idx.tolist() == hit and out == b"".join(LINES[d] for d in hit)
        for source in (False, True):
            sidx, sp, low = f.SpansLines(data, w, source=source)
            assert low and sidx.tolist() == hit
            assert [sorted(x) for x in sp] == [sorted(spans[d]) for d in hit], source    # (the lowered lines have the caller's lengths here)
        masked, _ = f.RedactLines(data, w, source=True)
        own, o = bytearray(data), 0
        for d, ln in enumerate(LINES):
            if d in hit:
                for s, t, _ in spans[d]:
                    own[o + s:o + t] = b"*" * (t - s)
            o += len(ln)
        assert masked == bytes(own)
        marked, _ = f.HighlightLines(data, b"[", b"]", w)
        if whole:
            assert b"us[he]rs" not in marked and b"ushers [he] [she] [hers]" in marked and b"concatenate [cat]" in marked
        else:
            assert b"u[shers] [he] [she] [hers]" in marked and b"con[cat]e[na]te [cat]" in marked
        got_stats, _ = f.TermStatsLines(data, w)
        assert got_stats == stats
        all_occ, _ = f.TermStatsLines(data, kept=False)
        ref_all = {}
        for d, doc in enumerate(ln.lower() for ln in LINES):
            for k in KEYWORDS:
                n = sum(1 for s in W.occurrences(doc, k) if not whole or W.kept(doc, s, s + len(k)))
                if n:
                    o, c, first = ref_all.get(k, (0, 0, d))
                    ref_all[k] = (o + n, c + 1, first)
        assert all_occ == ref_all
        assert f.CountExpressions(data).tolist() == [int((rows[:, 0] >> i & 1).sum()) for i in range(len(EXPRS))]
        # the option switched on the same finder
        f.whole_words = not whole
        assert (f.ProcessTexts(LINES) == finder_reference(LINES, not whole)[0]).all()
    finally:
        f.close()


def test_finder_batch_that_leaves_ascii():
    """keyword `école` over `ÉCOLE école Écolen`: the batch is lowered on the device, scanned again and filtered on the lowered text"""
    f = Finder(GpuEngine.__new__(GpuEngine), EmptyRgxEngine(), False, whole_words=True)
    g = Finder(GpuEngine.__new__(GpuEngine), EmptyRgxEngine(), False)
    try:
        for x in (f, g):
            x.AddExpressions(['"école"', '"cole"'])
        lines = ["ÉCOLE école Écolen\n".encode(), "Écolen\n".encode(), b"cole\n", "ÉCOLE\n".encode()]
        data = b"".join(lines)
        before = f.lowered_batches() if hasattr(f, "lowered_batches") else None
        off, bm = f.ProcessLines(data)
        assert bm.ravel().tolist() == [1, 0, 2, 1]
        assert g.ProcessLines(data)[1].ravel().tolist() == [3, 3, 2, 3]
        if before is not None:
            assert f.lowered_batches()[0] == before[0] + 1
        idx, spans, low = f.SpansLines(data, source=True)
        kw = "école".encode()
        assert low and idx.tolist() == [0, 2, 3] and spans == [[(0, 6, kw), (7, 13, kw)], [(0, 4, b"cole")], [(0, 6, kw)]]
        assert (f.ProcessTexts(lines) == bm).all()
    finally:
        f.close()
        g.close()


class _Foreign:
    def BuildEngine(self, keywords, caseSensitive):
        self.kw = list(keywords)

    def FindSubstrings(self, text):
        return []


def test_finder_unsupported_combinations():
    cases = {"regex terms": lambda: Finder(GpuEngine.__new__(GpuEngine), PyRegexpEngine(), True, whole_words=True),
             "a foreign substring engine": lambda: Finder(_Foreign(), EmptyRgxEngine(), True, whole_words=True),
             "several devices": lambda: Finder(GpuEngine.__new__(GpuEngine), EmptyRgxEngine(), True, devices=[0, 0], whole_words=True)}
    for why, make in cases.items():
        f = make()
        try:
            f.AddExpression('"he" and r"b+"' if why == "regex terms" else '"he"')
            for call in (lambda: f.ProcessTexts([b"he"]), lambda: f.ProcessText("he"), lambda: f.ProcessTextsSparse([b"he"]),
                         lambda: f.SelectLines(b"he\n"), lambda: f.SpansLines(b"he\n"), lambda: f.TermStatsLines(b"he\n")):
                with pytest.raises(FinderError) as ei:
                    call()
                assert ei.value.code == W.E_UNSUPPORTED, why
            with pytest.raises(FinderError) as ei:
                f.ProcessTexts([b"he"])
            assert why in str(ei.value)
        finally:
            f.close()
    # the pipelined form
    f = new_finder(True, case_sensitive=True)
    try:
        r = Resident([b"he"])
        bm = r.rows()
        torch.cuda.synchronize()
        with pytest.raises(FinderError) as ei:
            f.ProcessDeviceBegin(r.text.data_ptr(), r.off.data_ptr(), 1, bm.data_ptr())
        assert ei.value.code == W.E_UNSUPPORTED
        f.ProcessDevice(r.text.data_ptr(), r.off.data_ptr(), 1, bm.data_ptr())
        assert int(bm.cpu().numpy().view(np.uint32)[0, 0]) == 1
    finally:
        f.close()
