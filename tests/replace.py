"""Replace (gft_replace_spans_device): the reference, written from the contract in include/gft.h alone -- per document the spans'
intervals, sorted, united with plain loops, the smallest id per component, the replacements spliced into a `bytes` --, the fixed
cases at the borders of the kernels' walk (gft_debug_replace_shape), seeded random batches, and assert_not_vacuous(): the mutants
of the reference that the fixed cases must tell apart.  No tests in here and none of the code under test:
tests/test_replace_host.py and tests/test_gpu_replace.py use it."""
import functools

import numpy as np

REPLACE_MAX = 255
MAX_REPS = 65536
FULL = 0xFFFFFFFF
CHUNK, TRIP, TILE = 16, 1024, 4096                  # the copy's geometry as the header states it (checked against replace_shape by the tests)


class Case:
    """docs: list of bytes; spans: per document a list of (start, len, key); reps: the table, a list of bytes; key_rep: None or the
    key -> id list; keyed False: d_span_key is NULL and every span asks for id 0; lead: bytes in front of the first document"""

    def __init__(self, name, docs, spans, reps=(b"[X]",), key_rep=None, keyed=True, lead=0):
        assert len(docs) == len(spans)
        self.name, self.docs = name, [bytes(d) for d in docs]
        self.spans = [[(s[0], s[1], s[2] if len(s) > 2 else 0) for s in sp] for sp in spans]
        self.reps, self.key_rep, self.keyed, self.lead = [bytes(r) for r in reps], key_rep, keyed, lead

    def but(self, name, **kw):
        c = Case(name, self.docs, self.spans, self.reps, self.key_rep, self.keyed, self.lead)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def ids(self):
        """per document the id every span asks for"""
        def one(key):
            if not self.keyed:
                return 0
            return key if self.key_rep is None else self.key_rep[key]
        return [[one(k) for _, _, k in sp] for sp in self.spans]

    def arrays(self, fill=0x00, span_lead=0, span_tail=0):
        """(blob uint8, doc_off, span_off uint64, start, len, key uint32 -- key None when not keyed): the lead bytes hold `fill`.
        span_lead / span_tail: entries of the span arrays in front of the batch's spans (span_off[0] = span_lead) and behind
        them; they hold FULL -- a span, and a key, every call would refuse if it read it"""
        blob = bytes([fill]) * self.lead + b"".join(self.docs)
        off = np.zeros(len(self.docs) + 1, dtype=np.uint64)
        off[0] = self.lead
        if self.docs:
            off[1:] = self.lead + np.cumsum([len(d) for d in self.docs], dtype=np.uint64)
        so = np.full(len(self.docs) + 1, span_lead, dtype=np.uint64)
        if self.docs:
            so[1:] = span_lead + np.cumsum([len(s) for s in self.spans], dtype=np.uint64)
        flat = [x for s in self.spans for x in s]
        st, ln, ky = (np.array([FULL] * span_lead + [x[i] for x in flat] + [FULL] * span_tail, dtype=np.uint32) for i in range(3))
        return np.frombuffer(blob, dtype=np.uint8), off, so, st, ln, (ky if self.keyed else None)


def runs_of(spans, ids, touch=True, pick=None):
    """the connected components of the union of [start, start + len): a sorted list of [S, E, id] -- id the smallest of the
    component's spans (pick "first": of the first listed one; "left": of the leftmost, the first listed among equals)"""
    comps = []
    for lo, hi, k in sorted((a, a + n, k) for k, (a, n, _) in enumerate(spans)):
        if comps and (lo <= comps[-1][1] if touch else lo < comps[-1][1]):
            comps[-1][1] = max(comps[-1][1], hi)
            comps[-1][2].append(k)
        else:
            comps.append([lo, hi, [k]])
    out = []
    for S, E, ks in comps:
        if pick == "first":
            rid = ids[min(ks)]
        elif pick == "left":
            rid = ids[min(ks, key=lambda k: (spans[k][0], k))]
        else:
            rid = min(ids[k] for k in ks)
        out.append([S, E, rid])
    return out


def expected(case, mutant=None, span_lead=0):
    """a dict of what the call hands back under exact caps: n_runs, total, out (bytes), out_off, doc_run_off, run_new, run_len,
    run_rep (lists).  span_lead: the batch as arrays(fill, span_lead, ..) hands it over (only a mutant reads it)"""
    out, out_off, doc_run_off, run_new, run_len, run_rep = [], [0], [0], [], [], []
    total, open_end, k, drift = 0, False, 0, 0
    pick = {"first_listed_rep": "first", "leftmost_rep": "left"}.get(mutant)
    for doc, spans, ids in zip(case.docs, case.spans, case.ids()):
        comps = runs_of(spans, ids, touch=mutant != "no_touch", pick=pick)
        # first_from_k: "first span of its document" decided from k, the index behind the base, instead of span_lead + k -- true only
        # for k == 0 and, by accident, where k equals the absolute span_off[d]: with span_lead == 0 always, else hardly ever
        glue = mutant == "cross_doc" or (mutant == "first_from_k" and k not in (0, span_lead + k))
        k += len(spans)
        pieces, pos, cut, put = [], 0, 0, 0
        for i, (S, E, rid) in enumerate(comps):
            rep = case.reps[rid]
            if mutant == "empty_run_dropped" and S == E:
                rep = b""
            if i == 0 and glue and open_end and S == 0 and E > 0:
                rep = b""                                           # one run across the border: the replacement stands in front of it
            pieces += [doc[pos:S], rep]
            new = S - cut + (0 if mutant == "shift_by_run_len" else put) + (drift if mutant == "batch_rank" else 0)
            run_new.append(new)
            run_len.append(len(rep))
            run_rep.append(rid)
            cut += E - S
            put += len(rep)
            pos = E
        pieces.append(doc[pos:])
        drift += put - cut
        open_end = bool(comps) and comps[-1][1] == len(doc) and comps[-1][1] > comps[-1][0]
        out += pieces
        total += sum(len(p) for p in pieces)
        out_off.append(total)
        doc_run_off.append(len(run_new))
    return {"n_runs": len(run_new), "total": total, "out": b"".join(out), "out_off": out_off, "doc_run_off": doc_run_off, "run_new": run_new,
            "run_len": run_len, "run_rep": run_rep}


ARRAYS = ("out_off", "doc_run_off", "run_new", "run_len", "run_rep")


def same(got, want):
    return all(got[k] == want[k] for k in ("n_runs", "total", "out") + ARRAYS)


def _text(n, seed=7):
    """n seeded random printable bytes: a misplaced byte shows"""
    rng = np.random.RandomState(seed)
    return bytes(rng.randint(0x20, 0x7F, size=n, dtype=np.uint8).tolist())


def _rep(n, salt=0):
    return bytes((i * 7 + salt) % 94 + 33 for i in range(n))


def table_cases():
    t = _text(75)
    spans = [(0, 3), (10, 5), (30, 1), (70, 5)]
    base = Case("table", [t], [spans])
    cs = [base.but("rep_len_%d" % n, reps=[_rep(n)]) for n in (0, 1, 15, 16, 17, REPLACE_MAX)]
    cs.append(base.but("table_of_one", reps=[b"#"]))
    big = [b"<first>"] + [b"x"] * (MAX_REPS - 2) + [b"<last>"]
    cs.append(Case("table_65536", [t], [[(0, 3, 0), (10, 5, MAX_REPS - 1), (30, 1, MAX_REPS - 1), (70, 5, 0)]], reps=big))
    cs.append(Case("mixed_lengths", [t], [[(0, 3, 2), (10, 5, 0), (30, 1, 3), (70, 5, 1)]], reps=[b"", b"1", _rep(17), _rep(REPLACE_MAX, 5)]))
    return cs


def run_cases():
    t = _text(40, 3)
    R = [b"[A]", b"<bb>", b"", b"{dddd}"]
    return [
        Case("run_first_byte", [t], [[(0, 4)]]),
        Case("run_last_byte", [t], [[(36, 4)]]),
        Case("run_whole_doc", [t], [[(0, 40)]]),
        Case("run_whole_doc_deleted", [t, t], [[(0, 40)], [(3, 2)]], reps=[b""]),
        Case("empty_docs", [b"", t, b"", b""], [[], [(3, 3)], [(0, 0)], []]),
        Case("empty_run_alone", [t], [[(7, 0)]]),
        Case("empty_run_at_ends", [t], [[(0, 0), (40, 0)]]),
        Case("empty_run_touching", [t], [[(7, 0), (7, 3), (12, 0), (9, 3), (20, 2), (22, 0)]]),
        Case("empty_runs_deleted", [t], [[(0, 0), (7, 0), (40, 0)]], reps=[b""]),
        Case("touch_across_docs_deleted", [t[:10], t[10:20], t[20:30]], [[(8, 2)], [(0, 3), (8, 2)], [(0, 10)]], reps=[b""]),
        Case("touch_across_docs", [t[:10], t[10:20], t[20:30]], [[(8, 2)], [(0, 3), (8, 2)], [(0, 10)]]),
        Case("touch_across_empty_docs_deleted", [t[:10], b"", b"", t[10:20]], [[(8, 2)], [(0, 0)], [], [(0, 3)]], reps=[b""]),
        Case("docs_without_spans", [t, t, t, t], [[(1, 2)], [], [], [(30, 10)]]),
        Case("second_doc_ranks", [t, t], [[(1, 2), (5, 2), (9, 2)], [(1, 2), (5, 2)]], reps=[b"[longer]"]),
        Case("nested_ids", [t], [[(12, 2, 1), (10, 10, 3)]], reps=R),
        Case("overlap_ids", [t], [[(5, 10, 3), (10, 10, 0)]], reps=R),
        Case("repeated_ids", [t], [[(5, 5, 3), (5, 5, 1), (5, 5, 2)]], reps=R),
        Case("touching_ids", [t], [[(5, 5, 1), (10, 5, 0), (16, 2, 3)]], reps=R),
        # the scan's order, end ascending: the first listed span (12, 2) is not the leftmost (10, 10), and the smallest id is neither's
        Case("smallest_is_neither", [t], [[(12, 2, 3), (14, 3, 0), (10, 10, 1)]], reps=R),
        Case("key_rep_given", [t], [[(1, 2, 5), (6, 2, 0), (7, 4, 2), (20, 3, 4)]], reps=R, key_rep=[3, 0, 1, 0, 2, 1]),
        Case("key_is_id", [t], [[(1, 2, 3), (6, 2, 0), (7, 4, 2), (20, 3, 1)]], reps=R),
        Case("no_keys", [t], [[(1, 2, 3), (6, 2, 9), (20, 3, 77)]], reps=R, keyed=False),
        Case("no_docs", [], []),
        Case("no_spans", [t, t], [[], []], lead=5),
    ]


def placement_cases():
    """where the runs and the replacements fall in the output's 16-byte chunks, 1 KiB trips and 4 KiB tiles"""
    cs = []
    t = _text(2 * TILE + 100, 11)
    sixteen = [(40 + 2 * k, 1) for k in range(16)]
    cs.append(Case("sixteen_deleted", [t[:200]], [sixteen], reps=[b""]))          # an output chunk from sixteen places of the source
    cs.append(Case("sixteen_one_byte", [t[:200]], [sixteen], reps=[b"#"]))
    cs.append(Case("sixteen_17_bytes", [t[:200]], [sixteen], reps=[_rep(17)]))
    cs.append(Case("many_deleted_in_tile", [t[:900]], [[(k, 2) for k in range(0, 900, 3)]], reps=[b""]))
    cs.append(Case("many_runs_in_tile", [t[:600]], [[(k, 1, k % 3) for k in range(0, 600, 3)]], reps=[b"", b"{}", b"<abc>"]))
    cs.append(Case("straddle_chunk", [t[:120]], [[(30, 5)]], reps=[b"<em>"]))                      # over 30 .. 33
    cs.append(Case("straddle_trip", [t[:TRIP + 200]], [[(TRIP - 2, 8)]], reps=[b"[NAME]"]))
    cs.append(Case("straddle_tile", [t], [[(TILE - 2, 8), (2 * TILE - 14, 5)]], reps=[b"[NAME]"]))
    cs.append(Case("long_rep_over_tile", [t], [[(TILE - 100, 8)]], reps=[_rep(REPLACE_MAX, 3)]))
    cs.append(Case("deleted_run_over_tile", [t], [[(50, TILE + 500), (TILE + 600, 3)]], reps=[b""]))
    cs.append(Case("replaced_run_over_tile", [t], [[(50, TILE + 500), (TILE + 600, 3)]], reps=[b"<gone>"]))
    for lead in (0, 1, 5, 8, 15):                                   # the text at five residues of the 16-byte grid
        cs.append(Case("text_residue_%d" % lead, [t[:300], t[300:700]], [[(17, 4), (100, 30)], [(0, 1), (399, 1)]], lead=lead))
    for r in range(CHUNK):                                          # a run beginning at each residue
        cs.append(Case("residue_%d" % r, [t[:120]], [[(32 + r, 3, 1), (90, 2, 0)]], reps=[b"", b"<<>>"]))
    return cs


def count_cases(tile_spans, trip_tiles):
    """span counts round the borders of the run passes' walk, with heads on both sides of each border"""
    cs = []
    for n in (tile_spans - 1, tile_spans, tile_spans + 1, tile_spans * trip_tiles + 1):
        # spans of 2 bytes, 3 apart: every span is a head; then every fourth gap closed: runs of two spans
        spans = [(3 * k, 3 if k % 4 == 1 else 2, k % 3) for k in range(n)]
        cut = (3 * n + 5) // 2
        cut -= cut % 3                                              # a document border between two spans
        k0 = cut // 3
        d0, d1 = spans[:k0], [(a - cut, ln, ky) for a, ln, ky in spans[k0:]]
        L = 3 * n + 5
        t = (_text(997, 13) * (L // 997 + 1))[:L]
        cs.append(Case("spans_%d" % n, [t[:cut], t[cut:]], [d0, d1], reps=[b"", b"<b>", b"[four]"]))
    return cs


def fixed_cases():
    return table_cases() + run_cases() + placement_cases()


def random_cases(seed, n_cases=40):
    rng = np.random.RandomState(seed)
    cs = []
    for i in range(n_cases):
        n_reps = int(rng.randint(1, 6))
        reps = [bytes(rng.randint(1, 256, size=int(rng.choice([0, 0, 1, 2, 4, 15, 16, 17, 40]))).astype(np.uint8).tolist()) for _ in range(n_reps)]
        mode = int(rng.randint(0, 3))                               # 0: no keys; 1: the key is the id; 2: through key_rep
        n_keys = int(rng.randint(1, 9))
        key_rep = [int(rng.randint(0, n_reps)) for _ in range(n_keys)] if mode == 2 else None
        docs, spans = [], []
        for _ in range(rng.randint(0, 7)):
            L = int(rng.choice([0, 1, 5, 17, 40, 130]))
            docs.append(bytes(rng.randint(1, 256, size=L, dtype=np.uint16).astype(np.uint8).tolist()))
            s = []
            for _ in range(rng.randint(0, 9)):
                a = int(rng.randint(0, L + 1))
                s.append((a, int(rng.randint(0, min(L - a, 12) + 1)), int(rng.randint(0, n_keys if mode == 2 else n_reps))))
            spans.append(sorted(s, key=lambda x: (x[0] + x[1], x[0])))
        cs.append(Case("random_%d_%d" % (seed, i), docs, spans, reps=reps, key_rep=key_rep, keyed=mode != 0, lead=int(rng.randint(0, 40))))
    return cs


MUTANTS = ("first_listed_rep", "leftmost_rep", "no_touch", "cross_doc", "empty_run_dropped", "shift_by_run_len", "batch_rank")
# a wrong reading of the span base that only span_off[0] != 0 tells apart: "first span of its document" decided from k
BASE_MUTANTS = ("first_from_k",)


@functools.lru_cache(maxsize=None)
def assert_not_vacuous(span_lead=1):
    """every mutant of the reference is told apart from the reference by some fixed case.  The base mutant is the reference itself
    on every fixed case handed over with span_off[0] == 0 -- that is the gap -- and differs on some fixed case handed over behind
    span_lead entries.  Returns {mutant: the names of the fixed cases that catch it}"""
    cases = fixed_cases()
    told = {}
    for mutant in MUTANTS:
        told[mutant] = [c.name for c in cases if not same(expected(c, mutant), expected(c))]
        assert told[mutant], "no fixed case tells the mutant %r from the contract" % mutant
    for mutant in BASE_MUTANTS:
        blind = [c.name for c in cases if not same(expected(c, mutant), expected(c))]
        assert not blind, "the mutant %r shows without a span base on %r: it is no base mutant" % (mutant, blind)
        told[mutant] = [c.name for c in cases if not same(expected(c, mutant, span_lead), expected(c, None, span_lead))]
        assert told[mutant], "no fixed case behind a span base of %d tells the mutant %r from the contract" % (span_lead, mutant)
    # the smallest id of one case is neither its first listed span's nor its leftmost's
    assert "smallest_is_neither" in told["first_listed_rep"] and "smallest_is_neither" in told["leftmost_rep"]
    return told
