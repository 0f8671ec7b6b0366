"""Excerpts (gft_excerpt_spans_device): the reference, written from the contract in include/gft.h alone -- per document the
windows, sorted, united with plain loops, sliced out of a `bytes` --, the fixed cases at the borders of the kernels' walk
(gft_debug_excerpt_shape), seeded random batches, and assert_not_vacuous(): the mutants of the reference that the fixed cases must
tell apart.  No tests in here and none of the code under test: tests/test_excerpts_host.py and tests/test_gpu_excerpts.py use it."""
import bisect
import functools

import numpy as np

FULL = 0xFFFFFFFF


class Case:
    """docs: list of bytes; spans: per document a list of (start, len); lead: bytes in front of the first document (doc_off[0])"""

    def __init__(self, name, docs, spans, before, after, runes=True, lead=0):
        assert len(docs) == len(spans)
        self.name, self.docs, self.spans = name, [bytes(d) for d in docs], [list(s) for s in spans]
        self.before, self.after, self.runes, self.lead = before, after, runes, lead

    def but(self, name, **kw):
        c = Case(name, self.docs, self.spans, self.before, self.after, self.runes, self.lead)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def arrays(self, fill=0x00, span_lead=0, span_tail=0):
        """(blob uint8, doc_off, span_off uint64, start, len uint32): the lead bytes hold `fill`.  span_lead / span_tail: entries of
        the span arrays in front of the batch's spans (span_off[0] = span_lead) and behind them; they hold FULL, FULL -- a span
        every call would refuse if it read it"""
        blob = bytes([fill]) * self.lead + b"".join(self.docs)
        off = np.zeros(len(self.docs) + 1, dtype=np.uint64)
        off[0] = self.lead
        if self.docs:
            off[1:] = self.lead + np.cumsum([len(d) for d in self.docs], dtype=np.uint64)
        so = np.full(len(self.docs) + 1, span_lead, dtype=np.uint64)
        if self.docs:
            so[1:] = span_lead + np.cumsum([len(s) for s in self.spans], dtype=np.uint64)
        flat = [x for s in self.spans for x in s]
        st = np.array([FULL] * span_lead + [a for a, _ in flat] + [FULL] * span_tail, dtype=np.uint32)
        ln = np.array([FULL] * span_lead + [b for _, b in flat] + [FULL] * span_tail, dtype=np.uint32)
        return np.frombuffer(blob, dtype=np.uint8), off, so, st, ln


def _cont(b):
    return (b & 0xC0) == 0x80


def window(doc, start, length, before, after, runes, text=None, base=0):
    """the window of the contract, [lo, hi) of the document.  text / base: the mutant that snaps in the blob, not in the document"""
    L = len(doc)
    lo, hi = max(0, start - before), min(L, start + length + after)
    if runes:
        for _ in range(3):
            if text is None:
                if not (0 < lo < L and _cont(doc[lo])):
                    break
            elif not (base + lo > 0 and lo < L and _cont(text[base + lo])):
                break
            lo -= 1
        for _ in range(3):
            if not (hi < L and _cont(doc[hi])):
                break
            hi += 1
    return lo, hi


def expected(case, mutant=None, span_lead=0, span_tail=0):
    """a dict of what the call hands back under exact caps: n_exc, total, out (bytes), exc_off, exc_doc, exc_start, exc_span_off,
    span_rel, doc_exc_off (lists).  Excerpts in document order, inside a document by position.  span_lead / span_tail: the batch as
    arrays(fill, span_lead, span_tail) hands it over; the outputs are stated at the caller's indexes: exc_span_off absolute,
    span_rel of span_lead + spans + span_tail entries, None where the call must leave the entry as it was"""
    out, exc_off, exc_doc, exc_start, exc_span_off, span_rel, doc_exc_off = [], [0], [], [], [], [], [0]
    text = b"\xbf" * case.lead + b"".join(case.docs)
    base, s_base, total = case.lead, span_lead, 0
    heads = []                                                      # per span: 1 where an excerpt begins (the base mutants' rank)
    pending = None                                                  # the cross_doc mutant: the last excerpt, in blob positions
    for d, (doc, spans) in enumerate(zip(case.docs, case.spans)):
        wins = [window(doc, a, n, case.before, case.after, case.runes, text if mutant == "lead_snap" else None, base) for a, n in spans]
        comps = []
        for lo, hi in sorted(wins):
            if comps and (lo < comps[-1][1] if mutant == "no_touch" else lo <= comps[-1][1]):
                comps[-1][1] = max(comps[-1][1], hi)
            else:
                comps.append([lo, hi])
        members = [[] for _ in comps]
        firsts = [S for S, _ in comps]
        for k, (lo, hi) in enumerate(wins):
            i = bisect.bisect_right(firsts, lo) - 1                 # (the components are disjoint and do not touch: at most one holds it)
            assert comps[i][0] <= lo and hi <= comps[i][1], "the reference's own premise: a window lies in one component"
            members[i].append(k)
        for (S, E), mem in zip(comps, members):
            assert mem == list(range(mem[0], mem[0] + len(mem))), "the reference's own premise: an excerpt is a run of spans"
            if mutant == "head_start":
                S = wins[mem[0]][0]
            # first_from_k: "first span of its document" decided from k, the index behind the base, instead of span_lead + k -- true
            # only for k == 0 and, by accident, where k equals the absolute span_off[d]: with span_lead == 0 always, else hardly ever
            glue = mutant == "cross_doc" or (mutant == "first_from_k" and mem[0] == 0 and s_base - span_lead not in (0, s_base))
            heads += [0 if glue and pending is not None and pending == base + S and exc_doc else 1] + [0] * (len(mem) - 1)
            if glue and pending is not None and pending == base + S and exc_doc:
                # glue to the excerpt in front: it ended where this one begins in the blob
                out.append(doc[S:E])
                total += E - S
                exc_off[-1] = total
                for k in mem:
                    span_rel.append(0)
                pending = base + E
                continue
            exc_doc.append(d)
            exc_start.append(S)
            exc_span_off.append(s_base + mem[0])
            out.append(doc[max(S, 0):E] if S >= 0 else text[base + S:base + E])
            for k in mem:
                span_rel.append(spans[k][0] - S)
            total += E - S
            exc_off.append(total)
            pending = base + E
        base += len(doc)
        s_base += len(spans)
        doc_exc_off.append(len(exc_doc))
    exc_span_off.append(s_base)
    n = s_base - span_lead
    assert len(heads) == len(span_rel) == n
    if mutant == "rel_at_k":                                        # the parallel output written at k instead of span_lead + k
        span_rel = span_rel + [None] * (span_lead + span_tail)
    else:
        span_rel = [None] * span_lead + span_rel + [None] * span_tail
    if mutant == "eso_rebased":                                     # exc_span_off counted from the batch's first span
        exc_span_off = [v - span_lead for v in exc_span_off]
    if mutant == "deo_at_abs":                                      # the excerpts in front of span span_off[d], not span_off[d] - span_lead
        rank, so = [0], span_lead
        for h in heads:
            rank.append(rank[-1] + h)
        doc_exc_off = []
        for spans in [[]] + case.spans:
            so += len(spans)
            doc_exc_off.append(rank[min(so, n)])
    return {"n_exc": len(exc_doc), "total": total, "out": b"".join(out), "exc_off": exc_off, "exc_doc": exc_doc, "exc_start": exc_start,
            "exc_span_off": exc_span_off, "span_rel": span_rel, "doc_exc_off": doc_exc_off}


ARRAYS = ("exc_off", "exc_doc", "exc_start", "exc_span_off", "span_rel", "doc_exc_off")


def same(got, want, untouched=None):
    """None, or what differs first.  got: a dict with numpy arrays cut to their sizes and out as bytes.  untouched: the value an entry
    of span_rel holds where the reference says None (the call must leave it alone)"""
    if (got["n_exc"], got["total"]) != (want["n_exc"], want["total"]):
        return "n_exc, total: got %r, want %r" % ((got["n_exc"], got["total"]), (want["n_exc"], want["total"]))
    for k in ARRAYS:
        w = [untouched if v is None else v for v in want[k]] if k == "span_rel" else want[k]
        g, w = np.asarray(got[k]).astype(np.int64), np.asarray(w, dtype=np.int64)
        if g.shape != w.shape:
            return "%s: %d entries, want %d" % (k, g.size, w.size)
        if not np.array_equal(g, w):
            i = int(np.nonzero(g != w)[0][0])
            return "%s[%d]: got %d, want %d" % (k, i, g[i], w[i])
    if bytes(got["out"]) != want["out"]:
        return "the excerpts' bytes differ"
    return None


# ---- the fixed cases ---------------------------------------------------------------------------------------------------------
def _rand_bytes(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def runs_case(name, runs, per_doc=None, seed=1):
    """one-byte spans with before = after = 1: the spans of a run two bytes apart (their windows overlap), the runs ten apart (they
    do not).  per_doc: how many spans each document takes (None: one document)"""
    pos, p = [], 5
    for r in runs:
        for _ in range(r):
            pos.append(p)
            p += 2
        p += 8
    per_doc = per_doc or [len(pos)]
    assert sum(per_doc) == len(pos)
    docs, spans, k = [], [], 0
    for i, n in enumerate(per_doc):
        mine = pos[k:k + n]
        k += n
        lo = mine[0] - 3 if mine else 0
        hi = mine[-1] + 4 if mine else 3
        docs.append(_rand_bytes(hi - lo, seed + i))
        spans.append([(q - lo, 1) for q in mine])
    return Case(name, docs, spans, 1, 1)


def refusal_spans(case, k):
    """the two span lists of a one-document case that the call must refuse, each breaking ONE rule of the contract and keeping the
    other: `order` -- span k made longer, so that its end lies behind span k + 1's and still inside the document --, and `past` --
    the last span reaching one byte past the document's end, the ends still ascending"""
    spans, L = list(case.spans[0]), len(case.docs[0])
    ends = lambda s: [a + n for a, n in s]                          # noqa: E731
    descents = lambda s: [i for i, (p, q) in enumerate(zip(ends(s), ends(s)[1:])) if q < p]   # noqa: E731
    assert not descents(spans) and max(ends(spans)) <= L
    order = list(spans)
    order[k] = (spans[k][0], ends(spans)[k + 1] - spans[k][0] + 2)
    assert descents(order) == [k] and max(ends(order)) <= L, "the order case breaks the order alone"
    past = spans[:-1] + [(L - 1, 2)]
    assert not descents(past) and [e > L for e in ends(past)] == [False] * (len(past) - 1) + [True], "the past case breaks the span rule alone"
    return order, past


def rune_docs():
    euro, grin = "€".encode(), "😀".encode()
    return [b"ab" + euro + b"cd" + grin + b"ef\xc3\xa9gh", b"xy" + b"\x80\x81\x82\x83\x84" + b"zw", b"\x80\x81\x82\x83\x84q" + grin[1:],
            b"q" + grin + b"\xbf\xbf\xbf\xbf\xbf", grin[1:] + b"k" + euro[:2], b"\xbf"]


@functools.lru_cache(maxsize=None)
def fixed_cases(tile, trip):
    """the smallest shapes at which the passes can go wrong; tile: the spans of a tile, trip: the tiles of a carry trip"""
    T, C = tile, trip
    body = _rand_bytes(200, 7)
    cases = []
    for gap in (0, 1, -1):
        cases.append(Case("gap %d" % gap, [body], [[(10, 3), (21 + gap, 2)]], 4, 4, runes=False))
    cases.append(Case("clipped at both ends", [body], [[(1, 2), (197, 2)]], 10, 10))
    cases.append(Case("before = after = 0", [body], [[(0, 1), (5, 3), (8, 2), (11, 0), (199, 1)]], 0, 0, runes=False))
    cases.append(Case("the whole document", [body, b"", body[:30]], [[(50, 2), (90, 1)], [], [(3, 1)]], FULL, FULL))
    cases.append(Case("a document of no bytes", [b"abc", b"", b"", b"de"], [[(1, 1)], [(0, 0), (0, 0)], [], [(0, 2)]], 2, 2))
    cases.append(Case("documents without spans between", [body[:20], body[20:40], body[40:70], body[70:75], body[75:100]],
                      [[], [(3, 2)], [], [], [(1, 1), (9, 4)]], 3, 3))
    cases.append(Case("windows touch in the blob", [body[:50], body[50:90], body[90:120]], [[(45, 2)], [(1, 2), (37, 1)], [(0, 1)]], 8, 8,
                      runes=False))
    cases.append(Case("no spans at all", [body[:10], b"", body[10:20]], [[], [], []], 5, 5))
    cases.append(runs_case("a run ends at a tile border", [T - 100, 100, 40]))
    cases.append(runs_case("a run crosses a tile border", [T - 56, 100, 40]))
    cases.append(runs_case("a run covers three tiles", [100, 3 * T + 50, 30]))
    cases.append(runs_case("a document border on a tile border", [T - 2, 2 + 3, 20], per_doc=[T, 23]))
    cases.append(runs_case("a second carry trip", [3] * (T * C // 3) + [T * C + 1 - 3 * (T * C // 3)]))
    # a long keyword that ends late: its window starts before every earlier span's, a tile away from the head
    n_short = T + 44
    short = [(1000 + 4 * i, 1) for i in range(n_short)]
    end = short[-1][0] + 1
    cases.append(Case("the suffix minimum reaches the head", [_rand_bytes(end + 500, 9)], [[(10, 2)] + short + [(500, end + 100 - 500)]], 1, 1,
                      runes=False))
    cases.append(Case("a later span reaches further back", [body], [[(100, 2), (60, 50), (120, 1)]], 3, 3, runes=False))
    docs = rune_docs()
    every = [(d, i) for d in docs for i in range(len(d))]
    for b, a in ((0, 0), (1, 1), (2, 3)):
        cases.append(Case("rune snap %d/%d" % (b, a), [d for d, _ in every], [[(i, 1)] for _, i in every], b, a))
    cases.append(Case("rune snap, len 0", [d for d, _ in every], [[(i, 0)] for _, i in every], 0, 0))
    cases.append(cases[-3].but("rune snap off", runes=False))
    cases.append(Case("a lead byte is not the document's", [b"ab\x80", b"\x80\x80xyz", b"\xbf\xbf"], [[(1, 1)], [(1, 1)], [(1, 1)]], 1, 0, lead=3))
    cases.append(Case("excerpts of 1 byte", [body], [[(i, 1) for i in range(0, 200, 3)]], 0, 0, runes=False))
    cases.append(Case("excerpts of 15, 16 and 17 bytes", [body] * 3, [[(3, 15), (30, 16), (60, 17)], [(0, 16), (20, 17), (40, 15)], [(1, 17)]], 0, 0,
                      runes=False))
    big = _rand_bytes(6000, 11)
    cases.append(Case("one excerpt past the copy's tile", [body[:40], big, body[40:90]], [[(5, 1), (30, 2)], [(100, 5000)], [(7, 3), (44, 1)]], 2, 2,
                      runes=False))
    cases.append(cases[3].but("doc_off[0] != 0", lead=37))
    return tuple(cases)


ALPHABET = [b"a", b"b", b" ", b"K", "é".encode(), "€".encode(), "😀".encode(), "İ".encode(), b"\x80", b"\xbf", b"\xff", b"\xe2\x82", b"\xf0\x9f"]


@functools.lru_cache(maxsize=None)
def random_cases(n=60, seed=2024):
    rng = np.random.default_rng(seed)
    cases = []
    for i in range(n):
        docs, spans = [], []
        for _ in range(int(rng.integers(1, 40))):
            doc = b"".join(ALPHABET[int(k)] for k in rng.integers(0, len(ALPHABET), int(rng.integers(0, 120))))
            if rng.random() < 0.15:
                doc = b""
            ends = np.sort(rng.integers(0, len(doc) + 1, int(rng.integers(0, 12)) if rng.random() < 0.8 else 0))
            s = []
            for e in ends.tolist():
                n_ = int(rng.integers(0, min(e, 9) + 1))
                s.append((e - n_, n_))
            docs.append(doc)
            spans.append(s)
        cases.append(Case("random %d" % i, docs, spans, int(rng.integers(0, 12)), int(rng.integers(0, 12)), bool(rng.random() < 0.6),
                          lead=int(rng.integers(0, 5))))
    # a batch of more than a tile of spans
    docs, spans = [], []
    for d in range(90):
        doc = b"".join(ALPHABET[int(k)] for k in rng.integers(0, len(ALPHABET), 300))
        ends = np.sort(rng.integers(0, len(doc) + 1, 9))
        docs.append(doc)
        spans.append([(e - min(e, 3), min(e, 3)) for e in ends.tolist()])
    cases.append(Case("random, several tiles", docs, spans, 6, 9, True, lead=2))
    return tuple(cases)


MUTANTS = ("no_touch", "cross_doc", "lead_snap", "head_start")
# wrong readings of the span base that only span_off[0] != 0 tells apart: the parallel output written at k instead of s0 + k;
# exc_span_off rebased to 0; "first span of its document" decided from k; doc_exc_off read at span_off[d] instead of span_off[d] - s0
BASE_MUTANTS = ("rel_at_k", "eso_rebased", "first_from_k", "deo_at_abs")


def assert_not_vacuous(tile, trip, span_lead=1, span_tail=1):
    """every mutant of the reference differs from the reference on some fixed case: the cases can tell them apart.  The base mutants
    are the reference itself on every fixed case handed over with span_off[0] == 0 -- that is the gap -- and differ on some fixed
    case handed over behind span_lead entries.  Returns {mutant: the names of the fixed cases that catch it}"""
    small = [c for c in fixed_cases(tile, trip) if len(c.docs) < 500 and sum(map(len, c.spans)) < 2000]
    told = {}
    for m in MUTANTS:
        told[m] = [c.name for c in small if _differs(c, m)]
        assert told[m], "no fixed case tells the mutant %r from the contract" % m
    for m in BASE_MUTANTS:
        blind = [c.name for c in small if _differs(c, m)]
        assert not blind, "the mutant %r shows without a span base on %r: it is no base mutant" % (m, blind)
        told[m] = [c.name for c in small if _differs(c, m, span_lead, span_tail)]
        assert told[m], "no fixed case behind a span base of %d tells the mutant %r from the contract" % (span_lead, m)
    return told


def _differs(case, mutant, span_lead=0, span_tail=0):
    try:
        got = expected(case, mutant, span_lead, span_tail)
    except (AssertionError, IndexError):                            # (the mutant breaks the reference's own premises: it differs)
        return True
    want = expected(case, None, span_lead, span_tail)
    return any(got[k] != want[k] for k in want)
