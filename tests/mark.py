"""Highlight (gft_mark_spans_device): the reference, written from the contract in include/gft.h alone -- per document the spans'
intervals, sorted, united with plain loops, the markers spliced into a `bytes`, span_new from the run's index in its document --,
the fixed cases at the borders of the kernels' walk (gft_debug_mark_shape), seeded random batches, and assert_not_vacuous(): the
mutants of the reference that the fixed cases must tell apart.  No tests in here and none of the code under test:
tests/test_mark_host.py and tests/test_gpu_mark.py use it."""
import bisect
import functools

import numpy as np

MARK_MAX = 255
FULL = 0xFFFFFFFF
CHUNK, TRIP, TILE = 16, 1024, 4096                  # the copy's geometry as the header states it (checked against mark_shape by the tests)


class Case:
    """docs: list of bytes; spans: per document a list of (start, len); lead: bytes in front of the first document (doc_off[0])"""

    def __init__(self, name, docs, spans, open=b"<em>", close=b"</em>", lead=0):
        assert len(docs) == len(spans)
        self.name, self.docs, self.spans = name, [bytes(d) for d in docs], [list(s) for s in spans]
        self.open, self.close, self.lead = bytes(open), bytes(close), lead

    def but(self, name, **kw):
        c = Case(name, self.docs, self.spans, self.open, self.close, self.lead)
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


def runs_of(spans, touch=True):
    """the connected components of the union of [start, start + len): a sorted list of [S, E]"""
    comps = []
    for lo, hi in sorted((a, a + n) for a, n in spans):
        if comps and (lo <= comps[-1][1] if touch else lo < comps[-1][1]):
            comps[-1][1] = max(comps[-1][1], hi)
        else:
            comps.append([lo, hi])
    return comps


def mark_doc(doc, spans, open, close, mutant=None):
    """one document: (marked bytes, span_new per span, runs)"""
    comps = runs_of(spans, touch=mutant != "no_touch")
    pieces, pos = [], 0
    for S, E in comps:
        pieces.append(doc[pos:S])
        if mutant == "empty_run_dropped" and S == E:
            pass
        elif mutant == "close_early" and E > S:
            pieces += [open, doc[S:E - 1], close, doc[E - 1:E]]
        else:
            pieces += [open, doc[S:E], close]
        pos = E
    pieces.append(doc[pos:])
    new, firsts = [], [S for S, _ in comps]
    for a, n in spans:
        r = bisect.bisect_right(firsts, a) - 1                      # (the runs are apart: the last that begins at or before it)
        new.append(a + (r + 1) * len(open) + r * len(close))
    return pieces, new, comps


def expected(case, mutant=None, span_lead=0, span_tail=0):
    """a dict of what the call hands back under an exact cap: n_runs, total, out (bytes), out_off, span_new, doc_run_off (lists).
    span_lead / span_tail: the batch as arrays(fill, span_lead, span_tail) hands it over; span_new is stated at the caller's
    indexes, span_lead + spans + span_tail entries, None where the call must leave the entry as it was"""
    out, out_off, span_new, doc_run_off = [], [0], [], [0]
    n_runs, total, open_end = 0, 0, False
    heads, k = [], 0                                                # per span: 1 where a run begins (the base mutants' rank)
    for doc, spans in zip(case.docs, case.spans):
        pieces, new, comps = mark_doc(doc, spans, case.open, case.close, mutant)
        firsts, seen = [S for S, _ in comps], set()
        for a, _ in spans:
            r = bisect.bisect_right(firsts, a) - 1
            heads.append(0 if r in seen else 1)
            seen.add(r)
        if mutant == "batch_rank":
            new = [v + n_runs * (len(case.open) + len(case.close)) for v in new]
        # first_from_k: "first span of its document" decided from k, the index behind the base, instead of span_lead + k -- true only
        # for k == 0 and, by accident, where k equals the absolute span_off[d]: with span_lead == 0 always, else hardly ever
        glue = mutant == "cross_doc" or (mutant == "first_from_k" and k not in (0, span_lead + k))
        k += len(spans)
        if glue and open_end and comps and comps[0][0] == 0 and comps[0][1] > 0:
            # the run in front ended at its document's end and this one begins at its document's start: one run across the border
            assert out[-2] == case.close and pieces[1] == case.open
            total -= len(out[-2]) + len(pieces[1])
            out[-2] = pieces[1] = b""
        open_end = bool(comps) and comps[-1][1] == len(doc) and comps[-1][1] > comps[-1][0]
        out += pieces
        span_new += new
        n_runs += len(comps)
        total += sum(len(p) for p in pieces)
        out_off.append(total)
        doc_run_off.append(n_runs)
    if mutant == "new_at_k":                                        # the parallel output written at k instead of span_lead + k
        span_new = span_new + [None] * (span_lead + span_tail)
    else:
        span_new = [None] * span_lead + span_new + [None] * span_tail
    if mutant == "dro_at_abs":                                      # the runs in front of span span_off[d], not span_off[d] - span_lead
        rank, so, both = [0], span_lead, len(case.open) + len(case.close)
        for h in heads:
            rank.append(rank[-1] + h)
        was, doc_run_off = doc_run_off, []
        for spans in [[]] + case.spans:
            so += len(spans)
            doc_run_off.append(rank[min(so, len(heads))])
        out_off = [o + (r - w) * both for o, r, w in zip(out_off, doc_run_off, was)]
    return {"n_runs": n_runs, "total": total, "out": b"".join(out), "out_off": out_off, "span_new": span_new, "doc_run_off": doc_run_off}


ARRAYS = ("out_off", "span_new", "doc_run_off")


def same(got, want):
    return all(got[k] == want[k] for k in ("n_runs", "total", "out") + ARRAYS)


def _text(n, seed=7):
    """n seeded random printable bytes: a misplaced byte shows"""
    rng = np.random.RandomState(seed)
    return bytes(rng.randint(0x20, 0x7F, size=n, dtype=np.uint8).tolist())


def marker_cases():
    t = _text(75)
    spans = [(0, 3), (10, 5), (30, 1), (70, 5)]
    base = Case("markers", [t], [spans])
    cs = []
    for n in (0, 1, 15, 16, 17, MARK_MAX):
        o, c = bytes(range(0x41, 0x41 + n)) if n < 60 else bytes((i % 200) + 33 for i in range(n)), bytes((255 - i) % 251 + 1 for i in range(n))
        cs.append(base.but("markers_len_%d" % n, open=o, close=c))
    cs += [base.but("open_only", open=b"[[", close=b""), base.but("close_only", open=b"", close=b"]]"),
           base.but("both_empty", open=b"", close=b"")]
    return cs


def run_cases():
    t = _text(40, 3)
    return [
        Case("run_first_byte", [t], [[(0, 4)]]),
        Case("run_last_byte", [t], [[(36, 4)]]),
        Case("run_whole_doc", [t], [[(0, 40)]]),
        Case("one_byte_runs", [t], [[(k, 1) for k in range(0, 40, 2)]], open=b"<", close=b">"),
        Case("nested", [t], [[(12, 2), (10, 10)]]),
        Case("overlap", [t], [[(5, 10), (10, 10)]]),
        Case("repeated", [t], [[(5, 5), (5, 5), (5, 5)]]),
        Case("touching", [t], [[(5, 5), (10, 5), (16, 2)]]),
        Case("empty_run_alone", [t], [[(7, 0)]]),
        Case("empty_run_touching", [t], [[(7, 0), (7, 3), (12, 0), (9, 3), (20, 2), (22, 0)]]),
        Case("empty_run_at_ends", [t], [[(0, 0), (40, 0)]]),
        Case("empty_docs", [b"", t, b"", b""], [[], [(3, 3)], [(0, 0)], []]),
        Case("docs_without_spans", [t, t, t, t], [[(1, 2)], [], [], [(30, 10)]]),
        Case("touch_across_docs", [t[:10], t[10:20], t[20:30]], [[(8, 2)], [(0, 3), (8, 2)], [(0, 10)]]),
        Case("second_doc_ranks", [t, t], [[(1, 2), (5, 2), (9, 2)], [(1, 2), (5, 2)]]),
        Case("no_docs", [], []),
        Case("no_spans", [t, t], [[], []], lead=5),
    ]


def placement_cases():
    """where the insertions fall in the output's 16-byte chunks, 1 KiB trips and 4 KiB tiles"""
    cs = []
    t = _text(2 * TILE + 100, 11)
    for r in range(CHUNK):                                          # the first insertion begins at output position 32 + r
        cs.append(Case("residue_%d" % r, [t[:120]], [[(32 + r, 3), (90, 2)]], open=b"<<", close=b">>"))
    cs.append(Case("straddle_chunk", [t[:120]], [[(30, 5)]], open=b"<em>", close=b"</em>"))              # open over 30 .. 33
    cs.append(Case("straddle_trip", [t[:TRIP + 200]], [[(TRIP - 2, 8)]], open=b"<em>", close=b"</em>"))
    cs.append(Case("straddle_tile", [t], [[(TILE - 2, 8), (2 * TILE - 14, 5)]], open=b"<em>", close=b"</em>"))
    cs.append(Case("long_marker_over_tile", [t], [[(TILE - 100, 8)]], open=bytes(range(1, 256)), close=bytes(range(255, 0, -1))))
    for lead in (0, 1, 5, 8, 15):                                   # the text at five residues of the 16-byte grid
        cs.append(Case("text_residue_%d" % lead, [t[:300], t[300:700]], [[(17, 4), (100, 30)], [(0, 1), (399, 1)]], lead=lead))
    cs.append(Case("many_insertions_in_tile", [t[:600]], [[(k, 1) for k in range(0, 600, 3)]], open=b"{", close=b"}"))
    return cs


def count_cases(tile_spans, trip_tiles):
    """span counts round the borders of the run passes' walk, with heads on both sides of each border"""
    cs = []
    for n in (tile_spans - 1, tile_spans, tile_spans + 1, tile_spans * trip_tiles + 1):
        # spans of 2 bytes, 3 apart: every span is a head; then every fourth gap closed: runs of two spans
        spans = [(3 * k, 3 if k % 4 == 1 else 2) for k in range(n)]
        cut = (3 * n + 5) // 2
        cut -= cut % 3                                              # a document border between two spans
        k0 = cut // 3
        d0, d1 = spans[:k0], [(a - cut, ln) for a, ln in spans[k0:]]
        L = 3 * n + 5
        t = (_text(997, 13) * (L // 997 + 1))[:L]
        cs.append(Case("spans_%d" % n, [t[:cut], t[cut:]], [d0, d1], open=b"<b>", close=b"</b>"))
    return cs


def fixed_cases():
    return marker_cases() + run_cases() + placement_cases()


def random_cases(seed, n_cases=40):
    rng = np.random.RandomState(seed)
    cs = []
    for i in range(n_cases):
        docs, spans = [], []
        for _ in range(rng.randint(0, 7)):
            L = int(rng.choice([0, 1, 5, 17, 40, 130]))
            docs.append(bytes(rng.randint(1, 256, size=L, dtype=np.uint16).astype(np.uint8).tolist()))
            s = []
            for _ in range(rng.randint(0, 9)):
                a = int(rng.randint(0, L + 1))
                s.append((a, int(rng.randint(0, min(L - a, 12) + 1))))
            spans.append(sorted(s, key=lambda x: (x[0] + x[1], x[0])))
        ol, cl = (int(rng.choice([0, 1, 2, 4, 15, 16, 17, 40])) for _ in range(2))
        cs.append(Case("random_%d_%d" % (seed, i), docs, spans, open=bytes(rng.randint(1, 256, size=ol).astype(np.uint8).tolist()),
                       close=bytes(rng.randint(1, 256, size=cl).astype(np.uint8).tolist()), lead=int(rng.randint(0, 40))))
    return cs


MUTANTS = ("no_touch", "close_early", "batch_rank", "empty_run_dropped", "cross_doc")
# wrong readings of the span base that only span_off[0] != 0 tells apart: span_new written at k instead of s0 + k; "first span of its
# document" decided from k; doc_run_off (and out_off with it) read at span_off[d] instead of span_off[d] - s0
BASE_MUTANTS = ("new_at_k", "first_from_k", "dro_at_abs")


@functools.lru_cache(maxsize=None)
def assert_not_vacuous(span_lead=1, span_tail=1):
    """every mutant of the reference is told apart from the reference by some fixed case.  The base mutants are the reference itself
    on every fixed case handed over with span_off[0] == 0 -- that is the gap -- and differ on some fixed case handed over behind
    span_lead entries.  Returns {mutant: the names of the fixed cases that catch it}"""
    cases = fixed_cases()
    told = {}
    for mutant in MUTANTS:
        told[mutant] = [c.name for c in cases if not same(expected(c, mutant), expected(c))]
        assert told[mutant], "no fixed case tells the mutant %r from the contract" % mutant
    for mutant in BASE_MUTANTS:
        blind = [c.name for c in cases if not same(expected(c, mutant), expected(c))]
        assert not blind, "the mutant %r shows without a span base on %r: it is no base mutant" % (mutant, blind)
        told[mutant] = [c.name for c in cases if not same(expected(c, mutant, span_lead, span_tail), expected(c, None, span_lead, span_tail))]
        assert told[mutant], "no fixed case behind a span base of %d tells the mutant %r from the contract" % (span_lead, mutant)
    return told
