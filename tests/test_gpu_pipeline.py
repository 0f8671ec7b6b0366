"""Two batches in flight (gft_process_device_begin / _end, Finder.ProcessDeviceBegin / End: what bench.py's step() drives)
against the oracle, under every scan kernel: batches that overflow the match pool while another batch is in flight, a
younger batch that grows the pool inside _begin, the non-ASCII verdict each _end hands back, a pipelined Finder over text
that leaves ASCII, and seeded random schedules over all of it.  A batch that was accepted with matches dropped past the
pool shows up as a scan launch too few (gft_profile_read), whatever the kernel happened to drop."""
import ctypes as C
import random
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before libgft.so is loaded: both must share ONE HIP runtime, the one torch brings along)

from gofindthem_amd.finder import EmptyRgxEngine, Finder, GpuEngine
from helpers import tree_to_program
from oracle import dsl_ref
from oracle.pyoracle import Oracle, pack_strings

pytestmark = pytest.mark.gpu

FOLD = 1                                     # GFT_FOLD_ASCII


@pytest.fixture(params=["scan5", "scan3", "dfa"], autouse=True)
def scan_kernel(request, monkeypatch):
    """the three shipped scan kernels: scan5 and scan3 count pool slabs, the DFA kernel counts matches (GFT_SCAN_KERNEL is
    read when the engine is built)"""
    monkeypatch.setenv("GFT_SCAN_KERNEL", request.param)
    monkeypatch.delenv("GFT_SCAN_ORDERED", raising=False)
    return request.param


def _lib():
    from gofindthem_amd import _lib as lib
    return lib.load()


def _device_batch(texts):
    blob, off = pack_strings(texts)
    t = torch.from_numpy(np.concatenate([blob, np.zeros(64, np.uint8)])).cuda()      # 64 bytes of readable slack
    o = torch.from_numpy(off.astype(np.int64)).cuda()
    return t, o


def _keywords(exprs):
    kw = {}
    for e in exprs:
        kw.update(dict.fromkeys(dsl_ref.parse(e, False)[1]))
    return sorted(kw)


class Batch:
    """device text + offsets, the oracle's bitmap and the verdict gft_last_nonascii must give for it"""

    def __init__(self, texts, oracle, verdict=0, name=""):
        self.texts, self.n, self.verdict, self.name = texts, len(texts), verdict, name
        blob, off = pack_strings(texts)
        self.want = oracle.process(blob, off, fold=True)
        self.t, self.o = _device_batch(texts)

    def bitmap(self, words):
        return torch.zeros((max(self.n, 1), words), dtype=torch.int32, device="cuda")


def _check(bm, b, what=""):
    got = bm.cpu().numpy().astype(np.uint32)[:b.n]
    if not np.array_equal(got, b.want):
        bad = np.nonzero((got != b.want).any(axis=1))[0]
        raise AssertionError("%s%s: %d of %d rows differ from the oracle (first %s)" % (what, b.name, bad.size, b.n, bad[:5].tolist()))


# ---- a dictionary with dense and empty text ------------------------------------------------------------------------------
DENSE = "~^|`"                               # (no byte of the synthetic corpus)
DENSE_TERMS = [a + b for a in DENSE for b in DENSE] + [a + b + c for a in DENSE for b in DENSE for c in DENSE]
DENSE_EXPRS = (['"%s"' % t for t in DENSE_TERMS[::9]] +
               ['"%s" and not "%s"' % (DENSE_TERMS[16 + 5 * i], DENSE_TERMS[i]) for i in range(8)] +
               ['inord("%s" and "%s")' % (DENSE_TERMS[20 + 3 * i], DENSE_TERMS[40 + 3 * i]) for i in range(8)] +
               [" or ".join('"%s"' % t for t in DENSE_TERMS)])      # (every n-gram is in the dictionary)


@pytest.fixture(scope="module")
def corpus():
    """100 expressions over a 1 000-term dictionary and 25 over every 2- and 3-gram of a four-symbol alphabet: text over
    that alphabet has two matches per byte, so a batch of a megabyte or two is well beyond the 1 M-entry pool that small
    batches leave behind (under every kernel: scan3 sizes its pool by the waves the batch fills, up to 2 K entries per
    unit); filler text has no match at all"""
    from gofindthem_amd.workload import Workload, make_expressions
    w = Workload(1000)
    exprs = make_expressions(w.terms(), 100, inord_fraction=0.3, cover=True) + DENSE_EXPRS
    kw = _keywords(exprs)
    o = Oracle(kw)
    o.set_expressions(exprs, False)
    rng = np.random.default_rng(7)
    symbols = np.frombuffer(DENSE.encode(), np.uint8)

    def dense(n, nb=4000):
        return [row.tobytes().decode() for row in symbols[rng.integers(0, len(DENSE), size=(n, nb))]]

    filler = lambda n, nb: [("qqqq zzzz " * (nb // 10 + 1))[:nb - (d % 7)] for d in range(n)]   # noqa: E731
    words = (len(exprs) + 31) // 32
    warm = Batch(filler(400, 24), o, name="warm")
    big1 = Batch(dense(400), o, name="big1")             # 3.2 M matches: beyond the pool, inside the unit table
    big2 = Batch(dense(360), o, name="big2")             # (fewer matches than big1: the pool big1's rerun leaves holds them)
    small = Batch(dense(200), o, name="A")               # 1.6 M matches in 0.8 MB
    wide = Batch(filler(600, 112000), o, name="wide")    # more documents than the unit table, 67 MB: text / 16 > A's cursor
    assert big1.want.any(axis=1).all() and big2.want.any(axis=1).all()
    return dict(exprs=exprs, oracle=o, words=words, warm=warm, big1=big1, big2=big2, small=small, wide=wide, w=w, kw=kw,
                dense=dense)


def _warm_finder(corpus):
    f = Finder(GpuEngine(), EmptyRgxEngine(), False)
    f.AddExpressions(corpus["exprs"])
    warm, words = corpus["warm"], corpus["words"]
    bm = warm.bitmap(words)
    for _ in range(4):                      # sizes learnt, deferred, then the one-launch unit table
        f.ProcessDevice(warm.t.data_ptr(), warm.o.data_ptr(), warm.n, bm.data_ptr())
    _check(bm, warm)
    return f


def _scans(L, eh):
    ms, n = C.c_double(), C.c_uint64()
    assert L.gft_profile_read(eh, b"scan", C.byref(ms), C.byref(n)) == 0
    return n.value


class _Raw:
    """begin / end on the engine handle itself (ASCII folding), or through the Finder"""

    def __init__(self, f, engine_level):
        self.f, self.L, self.eh, self.engine_level = f, _lib(), f.engine_handle(), engine_level

    def begin(self, b, bm):
        if self.engine_level:
            assert self.L.gft_process_device_begin(self.eh, b.t.data_ptr(), b.o.data_ptr(), b.n, FOLD, None, bm.data_ptr()) == 0
        else:
            self.f.ProcessDeviceBegin(b.t.data_ptr(), b.o.data_ptr(), b.n, bm.data_ptr())

    def end(self):
        if self.engine_level:
            assert self.L.gft_process_device_end(self.eh) == 0
        else:
            self.f.ProcessDeviceEnd()


@pytest.mark.parametrize("level", ["engine", "finder"])
def test_two_overflowing_batches_in_flight(corpus, level):
    """begin(big1), begin(big2), end, end on a warmed engine: both outgrow the pool the small batches left behind.  big1's
    end grows the pool and runs big1 again; big2 ran with the OLD pool and dropped what lay past it, so it must be run again
    too, although the pool has meanwhile grown past big2's cursor (each big batch: two scan launches at least)."""
    f = _warm_finder(corpus)
    raw = _Raw(f, level == "engine")
    L, eh, words = raw.L, raw.eh, corpus["words"]
    big1, big2 = corpus["big1"], corpus["big2"]
    bm1, bm2 = big1.bitmap(words), big2.bitmap(words)
    L.gft_profile_enable(eh, 1)
    L.gft_profile_reset(eh)
    raw.begin(big1, bm1)
    raw.begin(big2, bm2)
    assert _scans(L, eh) == 2
    raw.end()
    after1 = _scans(L, eh)
    raw.end()
    after2 = _scans(L, eh)
    L.gft_profile_enable(eh, 0)
    _check(bm1, big1)
    _check(bm2, big2)
    assert after1 >= 3, "big1 was not scanned again after it overflowed the pool"
    assert after2 >= after1 + 1, "big2 overflowed the pool it was launched with and was accepted without a second scan"
    f.close()


def test_younger_batch_grows_the_pool_inside_begin(corpus):
    """begin(A), begin(B), end(A), end(B): A (dense, little text) is deferred and overflows; B has more documents than the
    unit table, so it completes inside its _begin -- and sizes the pool from its text (text / 16 entries), past A's
    cursor.  A ran with the smaller pool and must still be run again."""
    f = _warm_finder(corpus)
    raw = _Raw(f, True)
    L, eh, words = raw.L, raw.eh, corpus["words"]
    a, b = corpus["small"], corpus["wide"]
    bma, bmb = a.bitmap(words), b.bitmap(words)
    L.gft_profile_enable(eh, 1)
    L.gft_profile_reset(eh)
    raw.begin(a, bma)
    assert _scans(L, eh) == 1
    raw.begin(b, bmb)
    before = _scans(L, eh)
    raw.end()
    after = _scans(L, eh)
    raw.end()
    L.gft_profile_enable(eh, 0)
    _check(bma, a)
    _check(bmb, b)
    assert after >= before + 1, "A overflowed the pool it was launched with and was accepted without a second scan"
    f.close()


# ---- the verdict each _end hands back ------------------------------------------------------------------------------------
SMALL_EXPRS = ['"école"', '"ecole" or "straße"', '"la" and not "k"', 'inord("la" and "carte")']
CLASSES = {
    "ascii": (["ECOLE la", "k LA carte", "plain text", "la CARTE ecole"], 0),
    "latin1": (["vive la école", "LA STRAßE", "à la carte", "plain ECOLE"], 0),       # lower-case Latin-1: ASCII folding suffices
    "upper": (["Vive la École", "LA STRASSE École", "la carte", "k"], 1),             # upper-case É: strings.ToLower differs
}


def _engine(terms, exprs):
    from gofindthem_amd.engine import Engine
    eng = Engine()
    eng.build([t.encode() for t in terms])
    progs = []
    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 40000))          # (tree_to_program walks an OR chain of 4 500 leaves recursively)
    try:
        for e in exprs:
            tree = dsl_ref.parse(e, False)[0]
            progs.append(tree_to_program(tree, lambda lit: eng.term_id(lit)))
    finally:
        sys.setrecursionlimit(limit)
    eng.set_programs(progs)
    return eng


def _class_batch(kind, n, oracle):
    texts, v = CLASSES[kind]
    return Batch([texts[i % len(texts)] for i in range(n)], oracle, v, name="%s x %d" % (kind, n))


@pytest.fixture(scope="module")
def host_set():
    """a program set with one expression beyond the device solver (an INORD of 2 x 4 500 leaves): every batch takes the
    synchronous path inside _begin"""
    terms = ["w%04dq" % i for i in range(1400)]
    huge = "inord((%s) and (%s))" % (" or ".join('"%s"' % terms[i % 700] for i in range(4500)),
                                     " or ".join('"%s"' % terms[700 + i % 700] for i in range(4500)))
    exprs = SMALL_EXPRS + [huge]
    kw = _keywords(exprs)
    o = Oracle(kw)
    o.set_expressions(exprs, False)
    return kw, exprs, o


@pytest.mark.parametrize("setup", ["deferred", "fresh", "host_solved"])
def test_each_end_reports_its_own_verdict(setup, host_set):
    """begin X, begin Y, end -> gft_last_nonascii is X's verdict, end -> Y's (gft.h: ASCII 0, lower-case Latin-1 0,
    upper-case non-ASCII 1), for every ordered pair of the three classes, on engines where both batches are deferred, where
    they complete inside _begin (a fresh engine, a batch larger than the unit table) and where every batch takes the
    synchronous path (a host-solved expression)"""
    L = _lib()
    if setup == "host_solved":
        kw, exprs, o = host_set
    else:
        kw, exprs = _keywords(SMALL_EXPRS), SMALL_EXPRS
        o = Oracle(kw)
        o.set_expressions(exprs, False)
    words = (len(exprs) + 31) // 32
    batches = {k: _class_batch(k, 64, o) for k in CLASSES}
    firsts = {k: _class_batch(k, 4, o) for k in CLASSES}
    eng = None
    if setup != "fresh":
        eng = _engine(kw, exprs)
        warm = batches["ascii"]
        bm = warm.bitmap(words)
        for _ in range(3):
            eng.process_device(warm.t.data_ptr(), warm.o.data_ptr(), warm.n, bm.data_ptr(), fold=True)
        _check(bm, warm)
        if setup == "host_solved":
            assert L.gft_n_host_exprs(eng._h) == 1
    for x in CLASSES:
        for y in CLASSES:
            if setup == "fresh":
                eng = _engine(kw, exprs)
                bx, by = firsts[x], batches[y]      # the first batch of an engine, then one larger than its unit table
            else:
                bx, by = batches[x], batches[y]
            bmx, bmy = bx.bitmap(words), by.bitmap(words)
            for b, bm in ((bx, bmx), (by, bmy)):
                assert L.gft_process_device_begin(eng._h, b.t.data_ptr(), b.o.data_ptr(), b.n, FOLD, None, bm.data_ptr()) == 0
            assert L.gft_process_device_end(eng._h) == 0
            assert L.gft_last_nonascii(eng._h) == bx.verdict, "%s: end of %s (then %s)" % (setup, bx.name, by.name)
            assert L.gft_process_device_end(eng._h) == 0
            assert L.gft_last_nonascii(eng._h) == by.verdict, "%s: end of %s (after %s)" % (setup, by.name, bx.name)
            _check(bmx, bx, "%s, %s then %s: " % (setup, x, y))
            _check(bmy, by, "%s, %s then %s: " % (setup, x, y))
            if setup == "fresh":
                eng.close()
    if setup != "fresh":
        eng.close()


def test_synchronous_batch_between_complete_and_the_ends():
    """begin(A: upper-case non-ASCII), begin(B: ASCII), _complete, gft_process_device(C: lower-case Latin-1), end, end -- what
    the finder does when it repeats a batch beside younger ones in flight.  gft_last_nonascii right after the synchronous call
    is C's verdict; A and B kept theirs in their slots while C was judged, and each _end hands its own back."""
    L = _lib()
    kw = _keywords(SMALL_EXPRS)
    o = Oracle(kw)
    o.set_expressions(SMALL_EXPRS, False)
    words = 1
    a, b, c = (_class_batch(k, 4, o) for k in ("upper", "ascii", "latin1"))
    assert (a.verdict, b.verdict, c.verdict) == (1, 0, 0)
    eng = _engine(kw, SMALL_EXPRS)
    bma, bmb, bmc = a.bitmap(words), b.bitmap(words), c.bitmap(words)
    for _ in range(3):                      # sizes learnt: A and B are deferred
        eng.process_device(b.t.data_ptr(), b.o.data_ptr(), b.n, bmb.data_ptr(), fold=True)
    bmb.zero_()
    for x, bm in ((a, bma), (b, bmb)):
        assert L.gft_process_device_begin(eng._h, x.t.data_ptr(), x.o.data_ptr(), x.n, FOLD, None, bm.data_ptr()) == 0
    assert L.gft_process_device_complete(eng._h) == 0
    assert L.gft_process_device(eng._h, c.t.data_ptr(), c.o.data_ptr(), c.n, FOLD, None, bmc.data_ptr()) == 0
    assert L.gft_last_nonascii(eng._h) == c.verdict, "after the synchronous call"
    assert L.gft_process_device_end(eng._h) == 0
    assert L.gft_last_nonascii(eng._h) == a.verdict, "end of A"
    assert L.gft_process_device_end(eng._h) == 0
    assert L.gft_last_nonascii(eng._h) == b.verdict, "end of B"
    for x, bm in ((a, bma), (b, bmb), (c, bmc)):
        _check(bm, x)
    eng.close()


# ---- a pipelined Finder over text that leaves ASCII ------------------------------------------------------------------------
def test_pipelined_finder_over_mixed_text():
    """bench.py's step(): two result buffers, always one batch begun ahead of the one that ends.  A batch with upper-case
    non-ASCII text is repeated through the host's ToLower (finder.go:140-142) while the next batch is in flight -- also when
    two such batches follow each other.  Every bitmap equals the oracle over str.lower() text."""
    f = Finder(GpuEngine(), EmptyRgxEngine(), False)
    f.AddExpressions(SMALL_EXPRS)
    o = Oracle(_keywords(SMALL_EXPRS))
    o.set_expressions(SMALL_EXPRS, False)
    words = 1
    seq = ["ascii", "latin1", "upper", "ascii", "upper", "upper", "latin1", "ascii", "ascii", "upper", "latin1", "upper"]
    batches = []
    for i, k in enumerate(seq):
        texts = [CLASSES[k][0][(d + i) % 4] for d in range(200)]
        lb, lo = pack_strings([s.lower() for s in texts])
        want = o.process(lb, lo, fold=False)
        t, od = _device_batch(texts)
        batches.append((t, od, len(texts), want, k))
    bms = [torch.zeros((200, words), dtype=torch.int32, device="cuda") for _ in range(2)]
    begun = []

    def end_oldest():
        i, slot = begun.pop(0)
        f.ProcessDeviceEnd()
        got = bms[slot].cpu().numpy().astype(np.uint32)
        assert np.array_equal(got, batches[i][3]), "batch %d (%s)" % (i, batches[i][4])

    for i, b in enumerate(batches):
        slot = i % 2
        if any(s == slot for _, s in begun):
            end_oldest()
        bms[slot].zero_()
        f.ProcessDeviceBegin(b[0].data_ptr(), b[1].data_ptr(), b[2], bms[slot].data_ptr())
        begun.append((i, slot))
        while len(begun) > 1:
            end_oldest()
    while begun:
        end_oldest()
    f.close()


# ---- seeded random schedules ---------------------------------------------------------------------------------------------
KINDS = ["small", "heavy", "long_doc", "many_docs", "empty"]
FLAVOURS = {"ascii": ("", 0), "latin1": (" à la carte, straße", 0), "upper": (" École", 1)}


def test_random_schedules(scan_kernel, corpus):
    """about 30 batches of every kind -- small, match-heavy (the pool overflows), one document longer than a work unit (off
    the one-launch unit table), more documents than the unit table, empty -- in ASCII, lower-case Latin-1 or upper-case
    non-ASCII text, begun and ended in a random interleaving with at most two in flight; every _end is checked against the
    oracle and its verdict against the batch's text"""
    seed = {"scan5": 11, "scan3": 12, "dfa": 13}[scan_kernel]
    r = random.Random(seed)
    o, words, w = corpus["oracle"], corpus["words"], corpus["w"]
    text, off = w.docs_host(0, 600)
    base = [bytes(text[int(off[d]):int(off[d + 1])]).decode().encode("ascii", "ignore").decode() for d in range(600)]
    L = _lib()
    eng = _engine(corpus["kw"], corpus["exprs"])
    n_many, n_heavy = [0], [0]

    def make(kind, flav, i):
        extra, v = FLAVOURS[flav]
        if kind == "empty":
            return Batch([], o, 0, name="%d empty" % i)
        if kind == "heavy":
            n_heavy[0] += 1                                          # (1.6 x the last one: the pool overflows again)
            texts = [d + extra if k % 5 == 0 else d for k, d in enumerate(corpus["dense"](int(300 * 1.6 ** n_heavy[0])))]
        elif kind == "long_doc":
            k = r.randrange(20, 80)
            texts = [" ".join(base[k:k + 8])] + base[:k]            # 30 KB and more: several units
        elif kind == "many_docs":
            n_many[0] += 1
            texts = [base[d % 600][:60] for d in range(1000 * (1 << n_many[0]))]
        else:
            k = r.randrange(1, 200)
            texts = base[k:k + r.randrange(20, 300)]
        texts = list(texts)
        if extra and kind != "heavy":
            for d in range(0, len(texts), 7):
                texts[d] = texts[d] + extra
        return Batch(texts, o, v, name="%d %s/%s" % (i, kind, flav))

    schedule, inflight, log = [], [], []
    n_batches = 30
    i = 0
    try:
        while i < n_batches or inflight:
            can_begin = i < n_batches and len(inflight) < 2
            if can_begin and (not inflight or r.random() < 0.6):
                kind = r.choices(KINDS, weights=[6, 2, 2, 1, 1])[0]
                if (kind == "many_docs" and n_many[0] >= 3) or (kind == "heavy" and n_heavy[0] >= 3):
                    kind = "small"
                b = make(kind, r.choice(list(FLAVOURS)), i)
                bm = b.bitmap(words)
                log.append("begin " + b.name)
                assert L.gft_process_device_begin(eng._h, b.t.data_ptr(), b.o.data_ptr(), b.n, FOLD, None, bm.data_ptr()) == 0
                inflight.append((b, bm))
                i += 1
            else:
                b, bm = inflight.pop(0)
                log.append("end " + b.name)
                assert L.gft_process_device_end(eng._h) == 0, L.gft_last_error(eng._h)
                assert L.gft_last_nonascii(eng._h) == b.verdict, "verdict of " + b.name
                if b.n:
                    _check(bm, b)
            schedule.append(log[-1])
    except AssertionError as ex:
        raise AssertionError("seed %d, schedule: %s\n%s" % (seed, "; ".join(log), ex)) from ex
    finally:
        eng.close()
