"""gft_last_nonascii at every byte position of every judge (fold_cases.py): the verdict of a folded scan is decided by k_fold_safe
with k_fold_doc_edges (the DFA kernel's batches, and every unit that lists more pieces than its candidate list holds), inside
gft_scan3, and inside gft_scan5 in two ways (small and large alphabet).  Every violation of every kind, and every safe pair, lies
at every position around every border of those geometries, one document per call; gft_debug_last_fold_bits says which judge
answered, so that a sweep meant for a kernel's own judge cannot pass through the fallback unnoticed.  Then the other ways a batch
is scanned (gft_process_device, two batches in flight, gft_hit_spans_device) and the consequence for a case-insensitive Finder.
Expected verdicts are the reference's (fold_cases.rows_safe); every comparison is exact."""
import ctypes as C
import os
import time

import numpy as np
import pytest
import torch  # noqa: F401  (before libgft.so is loaded: both must share ONE HIP runtime, the one torch brings along)

import fold_cases as fc
from helpers import OP_UNIT

pytestmark = pytest.mark.gpu

FOLD = 1                                          # GFT_FOLD_ASCII
JUDGES = ("scan5-small", "scan5-large", "scan3", "dfa")
KERNEL = {"scan5-small": "scan5", "scan5-large": "scan5", "scan3": "scan3", "dfa": "dfa"}
SMALL = [b"abc", b"b", b"caf\xc3\xa9", b"stra\xc3\x9fe"]          # test_gpu_parity.test_fold_safety_is_decided_per_document's


def _L():
    from gofindthem_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def large():
    """the keywords of a word list over more than 32 byte classes (test_gpu_parity.test_large_alphabet_on_a_fresh_engine...)"""
    from gofindthem_amd.workload import Workload
    w = Workload(3000, alphabet="mixed")
    return sorted({t.decode("utf-8").lower().encode("utf-8") for t in w.terms()})


class Engines:
    """an engine per judge, built under the scan kernel it names (GFT_SCAN_KERNEL is read by gft_build)"""

    def __init__(self, large):
        self.made, self.large = {}, large

    def of(self, judge):
        if judge not in self.made:
            from gofindthem_amd.engine import Engine
            terms = self.large if judge == "scan5-large" else SMALL
            assert not _spelt(terms), (judge, _spelt(terms)[:5])
            old = os.environ.get("GFT_SCAN_KERNEL")
            os.environ["GFT_SCAN_KERNEL"] = KERNEL[judge]
            try:
                e = Engine()
                e.build(terms)
            finally:
                if old is None:
                    del os.environ["GFT_SCAN_KERNEL"]
                else:
                    os.environ["GFT_SCAN_KERNEL"] = old
            assert _L().gft_scan_kernel(e._h).decode() == KERNEL[judge], judge
            classes = len({b for t in terms for b in t}) + 1                 # (every byte of no keyword is one more class)
            assert classes > 48 if judge == "scan5-large" else classes <= 32, (judge, classes)
            e.set_programs([[OP_UNIT << 28 | 0], [OP_UNIT << 28 | 1]])
            self.made[judge] = e
        return self.made[judge]

    def close(self):
        for judge, e in self.made.items():
            if KERNEL[judge] == "scan5":                                     # (the geometry the lengths were chosen for)
                um = C.c_uint32()
                assert _L().gft_debug_learned_unit(e._h, C.byref(um), None) == 0 and um.value == fc.UNIT_MAX, (judge, um.value)
            e.close()
        self.made = {}


def _spelt(terms):
    """the keywords that the cases' text could spell at all (none: the unit size then stays at 8 192 bytes)"""
    text = bytes(fc._LETTERS).lower() + b"ajx" + b"".join(fc.VIOLATIONS.values()) + b"".join(fc.SAFE_PAIRS.values())
    return [t for t in terms if set(t) <= set(text)]


@pytest.fixture(scope="module")
def engines(large):
    es = Engines(large)
    yield es
    es.close()


class Dev:
    """a family's blob and offsets, resident"""

    def __init__(self, blob, off):
        self.t = torch.from_numpy(np.array(blob, dtype=np.uint8)).cuda()                      # (a copy: the families are read-only)
        self.o = torch.from_numpy(np.ascontiguousarray(off).astype(np.int64)).cuda()
        assert self.t.data_ptr() % 16 == 0 and self.o.data_ptr() % 8 == 0          # (residues on the 16-byte grid are off % 16)
        self.text, self.off = self.t.data_ptr(), self.o.data_ptr()


_DEV = {}


def _dev(key):
    if key not in _DEV:
        fam = fc.family(*key)
        _DEV[key] = Dev(fam.blob, fam.off)
    return fc.family(*key), _DEV[key]


def _scan(eng, dev, d, n=1, fold=True):
    """gft_scan_device over the documents d .. d + n of a resident family -> gft_last_nonascii"""
    from gofindthem_amd._lib import GftMatches
    m = GftMatches()
    eng._check(eng._L.gft_scan_device(eng._h, dev.text, dev.off + 8 * d, n, FOLD if fold else 0, C.byref(m)))
    return eng._L.gft_last_nonascii(eng._h)


def _bits(eng):
    b = C.c_uint32(99)
    assert eng._L.gft_debug_last_fold_bits(eng._h, C.byref(b)) == 0
    return b.value


def _route(eng):
    name = C.c_char_p()
    assert eng._L.gft_debug_last_unit_route(eng._h, C.byref(name)) == 0
    return name.value.decode()


def _check_bits(judge, filler, bits):
    """which judge answered an unsafe document.  ASCII filler: the violation is the only high byte of its unit, so a kernel that
    judges does (2); the DFA kernel never does (bit 0).  Dense filler: either the unit's list held its pieces (2) or it
    overflowed and k_fold_safe answered (bit 0) -- cand_cap follows the LDS the dictionary leaves, so both are right"""
    if judge == "dfa":
        return bits & 1
    if filler == "ascii":
        return bits == 2
    return bits == 2 or bits & 1


@pytest.mark.parametrize("key", fc.UNSAFE_FAMILIES, ids=fc.family_id)
@pytest.mark.parametrize("judge", JUDGES)
def test_unsafe_sweep(engines, judge, key):
    """every violation, ONE document per call (the verdict is an OR): 1, by the judge the case was made for; without folding 0"""
    eng = engines.of(judge)
    fam, dev = _dev(key)
    bad, seen, t0 = [], {}, time.perf_counter()
    for i, c in enumerate(fam.cases):
        got = _scan(eng, dev, c.doc)
        bits = _bits(eng)
        seen[bits] = seen.get(bits, 0) + 1
        raw = _scan(eng, dev, c.doc, fold=False)
        if got != int(fam.unsafe[i]) or raw != 0 or not _check_bits(judge, key[2], bits):
            bad.append((c.kind, c.p, "address %% 16 = %d" % ((int(fam.off[c.doc]) + c.p) % 16), "verdict %d, bits %d, unfolded %d" % (got, bits, raw)))
    print("%s %s: %d cases, bits seen %s, %.0f us a call" % (judge, fam.name, len(fam.cases), seen, (time.perf_counter() - t0) / (2 * len(fam.cases)) * 1e6))
    assert not bad, "%d of %d unsafe documents of %s under %s; the first: %s" % (len(bad), len(fam.cases), fam.name, judge, bad[:8])


@pytest.mark.parametrize("key", fc.SAFE_FAMILIES, ids=fc.family_id)
@pytest.mark.parametrize("judge", JUDGES)
def test_safe_sweep(engines, judge, key):
    """safe pairs at the same positions, cut by pieces, lanes, rounds and units: 0 for the family in one call and for every
    document by itself (a false 1 costs the batch a lowering pass)"""
    eng = engines.of(judge)
    fam, dev = _dev(key)
    whole = _scan(eng, dev, 0, fam.n_docs)
    whole_bits = _bits(eng)
    bad, seen = [], {}
    for i, c in enumerate(fam.cases):
        got = _scan(eng, dev, c.doc)
        bits = _bits(eng)
        seen[bits] = seen.get(bits, 0) + 1
        if got != int(fam.unsafe[i]) or (judge == "dfa" and not bits & 1):
            bad.append((c.kind, c.p, "address %% 16 = %d" % ((int(fam.off[c.doc]) + c.p) % 16), "verdict %d, bits %d" % (got, bits)))
    print("%s %s: %d cases, bits seen %s; the family in one call: bits %d" % (judge, fam.name, len(fam.cases), seen, whole_bits))
    spacers = [d for d in range(1, fam.n_docs, 2) if whole and _scan(eng, dev, d)]          # (asked only to explain a failure)
    assert not bad and not whole, "the family %s under %s: verdict %d (bits %d); %d of its documents alone, the first: %s; spacers %s" % (
        fam.name, judge, whole, whole_bits, len(bad), bad[:8], spacers[:8])


@pytest.mark.parametrize("judge", JUDGES)
def test_two_documents_whose_border_cuts_a_pair(engines, judge):
    """a document that ends in a lone lead in front of one that begins with a continuation byte, both in ONE batch: a pair that
    the rule accepts lies across the border, and only the look at every document's own first and last byte says 1"""
    eng = engines.of(judge)
    for filler in fc.FILLERS:
        fam, pairs = fc.rim_pairs(filler)
        _, dev = _dev(("rim", 0, filler))
        bad = []
        for d in pairs:
            got = _scan(eng, dev, d, 2)
            bits = _bits(eng)
            if got != 1 or not _check_bits(judge, filler, bits):
                bad.append((d, bytes(fam.doc(d)[-1:]).hex(), bytes(fam.doc(d + 1)[:1]).hex(), int(fam.off[d + 1]) % 16, got, bits))
        assert not bad, (judge, filler, len(bad), len(pairs), bad[:8])


# ---- the other ways a batch is scanned -------------------------------------------------------------------------------------
AROUND = 3                                        # safe dense documents on either side of the unsafe one


def _groups(n):
    """-> (blob, off, [(name, index of the batch's first document, reference's verdict)]): for every thinned case a batch of
    2 * AROUND + 1 documents -- the case between safe dense ones -- and in front of them all one batch of safe dense documents"""
    safe = fc.safe_family(n, "dense")
    around = [safe.doc(c.doc) for c in safe.cases[:: max(1, len(safe.cases) // (2 * AROUND + 1))]][:2 * AROUND + 1]
    docs, batches = list(around), [("all safe", 0, 0)]
    for filler in fc.FILLERS:
        fam, idx = fc.thinned(n, filler)
        for i in idx:
            c = fam.cases[i]
            batches.append(("%s %s at %d" % (fam.name, c.kind, c.p), len(docs), int(fam.unsafe[i])))
            docs += around[:AROUND] + [fam.doc(c.doc)] + around[AROUND:2 * AROUND]
    want = [int(not all(fc.doc_safe_np(d) for d in docs[b:b + 2 * AROUND + 1])) for _, b, _ in batches]
    assert want == [w for _, _, w in batches] and want[0] == 0 and all(want[1:])
    lens = np.asarray([len(d) for d in docs], dtype=np.uint64)
    off = np.concatenate([[fc.LEAD], fc.LEAD + np.cumsum(lens, dtype=np.uint64)]).astype(np.uint64)
    blob = np.concatenate([np.full(fc.LEAD, 0xC3, np.uint8)] + docs + [np.full(fc.SLACK, 0x89, np.uint8)])
    return blob, off, batches


@pytest.mark.parametrize("judge", JUDGES)
def test_the_other_ways_a_batch_is_scanned(engines, judge):
    """the thinned list -- every context-sensitive kind at piece bytes 0 and 15, at a unit border and at the document's end, in
    1 000 and 20 000 bytes -- through gft_process_device and gft_hit_spans_device, one document a call, and with two batches in
    flight, the unsafe document among safe dense ones, in both orders: each publishes the reference's verdict"""
    eng = engines.of(judge)
    L = eng._L
    routes, n_cases = set(), 0
    for n in (1000, 20000):
        # one document a call
        for filler in fc.FILLERS:
            fam, idx = fc.thinned(n, filler)
            _, dev = _dev(("unsafe", n, filler))
            kinds = {fam.cases[i].kind for i in idx}
            assert kinds == set(fc.SENSITIVE) and len(idx) >= 3 * len(kinds), (n, filler, len(idx))
            bm = torch.zeros((1, 1), dtype=torch.int32, device="cuda")
            total = C.c_uint64()
            for i in idx:
                c = fam.cases[i]
                eng.process_device(dev.text, dev.off + 8 * c.doc, 1, bm.data_ptr(), fold=True)
                got_p, bits_p = L.gft_last_nonascii(eng._h), _bits(eng)
                eng._check(L.gft_hit_spans_device(eng._h, dev.text, dev.off + 8 * c.doc, 1, FOLD, bm.data_ptr(), None, None, None, None, None, None,
                                                  0, C.byref(total)))
                got_s, bits_s = L.gft_last_nonascii(eng._h), _bits(eng)
                assert got_p == got_s == int(fam.unsafe[i]) == 1, (judge, fam.name, c, got_p, got_s)
                assert _check_bits(judge, filler, bits_p) and _check_bits(judge, filler, bits_s), (judge, fam.name, c, bits_p, bits_s)
                n_cases += 1
        # two batches in flight
        blob, off, batches = _groups(n)
        dev = Dev(blob, off)
        k = 2 * AROUND + 1
        bms = [torch.zeros((k, 1), dtype=torch.int32, device="cuda") for _ in range(2)]
        safe_first = batches[0][1]
        for name, first, want in batches[1:]:
            for order in ((first, safe_first), (safe_first, first)):
                for d, bm in zip(order, bms):
                    eng._check(L.gft_process_device_begin(eng._h, dev.text, dev.off + 8 * d, k, FOLD, None, bm.data_ptr()))
                    routes.add(_route(eng))
                for d in order:
                    eng._check(L.gft_process_device_end(eng._h))
                    assert L.gft_last_nonascii(eng._h) == (want if d == first else 0), (judge, n, name, "the unsafe batch first" if order[0] == first else "the safe batch first", _bits(eng))
    print("%s: %d documents through gft_process_device and gft_hit_spans_device; unit routes of the batches in flight: %s" % (judge, n_cases, sorted(routes)))
    assert {"deferred", "single"} <= routes, routes


# ---- the consequence ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["scan5", "scan3", "dfa"])
def test_a_finder_lowers_the_batch_that_holds_an_upper_case_rune(kernel, monkeypatch):
    """a case-insensitive Finder with the keyword "école": 64 safe dense documents and ONE that holds "École" -- C3 89 at the
    swept position -- and the keyword in no other spelling.  If the verdict were 0 the batch would not be lowered and the
    document not marked; the rows are the oracle's over the host's strings.ToLower of the documents"""
    from gofindthem_amd.finder import EmptyRgxEngine, Finder, GpuEngine
    from oracle.pyoracle import Oracle, pack_strings
    from tolower_cases import ref_lower
    monkeypatch.setenv("GFT_SCAN_KERNEL", kernel)
    exprs = ['"école"', '"keyword"']
    o = Oracle(sorted(["école".encode(), b"keyword"]))
    o.set_expressions(exprs, False)
    f = Finder(GpuEngine(), EmptyRgxEngine(), False)
    try:
        f.AddExpressions(exprs)
        lowered = 0
        for n in (1000, 20000):
            fam, idx = fc.thinned(n, "dense")
            ps = sorted({fam.cases[i].p for i in idx if fam.cases[i].kind == "C3 89" and fam.cases[i].p + 6 <= n} | {n - 6})      # (... and "École" ends the document)
            assert len(ps) >= 3
            safe = [fc.build_doc(n, "dense", 2 * d, b"KeyWord" if d % 5 == 0 else b"\xc3\xbf") for d in range(64)]
            assert all(map(fc.doc_safe_np, safe))
            for p in ps:
                doc = fc.build_doc(n, "dense", p, "École".encode())
                assert doc[p] == 0xC3 and doc[p + 1] == 0x89 and "école".encode() not in doc.tobytes() and not fc.doc_safe_np(doc)
                docs = [d.tobytes() for d in safe[:32] + [doc] + safe[32:]]
                dev = Dev(np.frombuffer(b"".join(docs) + bytes(64), dtype=np.uint8), np.concatenate([[0], np.cumsum([len(d) for d in docs])]))
                blob, off = pack_strings([ref_lower(d) for d in docs])
                want = o.process(blob, off, fold=False)
                assert want[32, 0] & 1 and sum(int(r[0]) & 1 for r in want) == 1 and sum(int(r[0]) >> 1 & 1 for r in want) == 13
                bm = torch.zeros((len(docs), 1), dtype=torch.int32, device="cuda")
                f.ProcessDevice(dev.text, dev.off, len(docs), bm.data_ptr())
                got = bm.cpu().numpy().astype(np.uint32)
                assert np.array_equal(got, want), (kernel, n, p, np.nonzero((got != want).any(axis=1))[0][:8])
                lowered += 1
                assert sum(f.lowered_batches()) == lowered, (kernel, n, p, f.lowered_batches())
    finally:
        f.close()
