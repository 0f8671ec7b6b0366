"""Batches for the tests of the hit spans and the redaction (test_spans_host.py: the kernels' walks on the host; test_gpu_spans.py:
the kernels): a reference written from the contract in include/gft.h that does not call the new code -- matches from the oracle's
scan, rows from the oracle's ProcessText, witness sets from a walk over the parsed trees, the filter and the geometry as plain
loops, the redaction by slicing a bytearray --, the fixed cases built from the kernels' own borders (gft_debug_spans_shape), seeded
random batches, and assert_not_vacuous().  The tail bits of every row's last word and of every mask are ones, so a walk that
honours them shows; the redaction's texts are random bytes, so a byte changed outside a span shows.  No tests in here."""
import collections
import functools

import numpy as np

from gofindthem_amd.engine import spans_shape
from helpers import tree_to_program
from oracle import dsl_ref
from oracle.pyoracle import POS_END, POS_START, Oracle

# ---- span cases ---------------------------------------------------------------------------------------------------------------
# docs: the documents' bytes; lead / slack: what lies in front of document 0 (doc_off[0] = len(lead)) and behind the last one on the
# device; at: the residue of the buffer's address.  rows: the bitmap [R, W] the call is given, row_idx: None or r(d); want: None or
# W words.  exprs: DSL strings, parsed case-sensitively unless fold
Case = collections.namedtuple("Case", "name exprs docs rows row_idx want pos_end fold lead slack at")


class Compiled:
    """what the expressions of a case give: the dictionary in the engine's order (unique keywords sorted bytewise), the postfix
    programs over its slots (regex literals are extra slots), the parsed trees"""

    def __init__(self, exprs, fold):
        self.trees, kws, rgx = [], {}, {}
        for e in exprs:
            t, k, r = dsl_ref.parse(e, not fold)
            self.trees.append(t)
            kws.update(dict.fromkeys(k))
            rgx.update(dict.fromkeys(r))
        self.terms = sorted({k.encode("utf-8") for k in kws})
        self.tid = {t: i for i, t in enumerate(self.terms)}
        self.regexes = [r for r in rgx if r.encode("utf-8") not in self.tid]
        self.n_terms, self.n_extra = len(self.terms), len(self.regexes)

        def slot_of(lit):
            b = lit.encode("utf-8")
            return self.tid[b] if b in self.tid else self.n_terms + self.regexes.index(lit)
        self.programs = [tree_to_program(t, slot_of) for t in self.trees]
        self.term_len = np.asarray([len(t) for t in self.terms], dtype=np.uint32)

    def witness_sets(self, not_is_witness=False):
        """P(i) as sets of term ids, by a walk over the trees: the keyword units outside every NOT.  not_is_witness: what a walk
        would answer that kept the units under a NOT (assert_not_vacuous)"""
        out = []
        for t in self.trees:
            p, stack = set(), [(t, False)]
            while stack:
                n, neg = stack.pop()
                if n is None:
                    continue
                if n.Type == dsl_ref.UNIT_EXPR:
                    b = n.Literal.encode("utf-8")
                    if b in self.tid and (not neg or not_is_witness):
                        p.add(self.tid[b])
                else:
                    below = neg or n.Type == dsl_ref.NOT_EXPR
                    stack += [(n.LExpr, below), (n.RExpr, below)]
            out.append(p)
        return out

    def witness_table(self):
        """the term -> expressions CSR the contract describes, from witness_sets"""
        sets = self.witness_sets()
        lists = [[i for i, p in enumerate(sets) if t in p] for t in range(self.n_terms)]
        off = np.zeros(self.n_terms + 1, dtype=np.uint64)
        if lists:
            off[1:] = np.cumsum([len(x) for x in lists], dtype=np.uint64)
        return off, np.asarray([i for x in lists for i in x], dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def compiled(exprs, fold):
    return Compiled(exprs, fold)


def packed(c):
    """(blob uint8 with the lead bytes in front, doc_off uint64 with doc_off[0] = len(lead))"""
    off = np.zeros(len(c.docs) + 1, dtype=np.uint64)
    off[0] = len(c.lead)
    if c.docs:
        off[1:] = len(c.lead) + np.cumsum([len(d) for d in c.docs], dtype=np.uint64)
    return np.frombuffer(c.lead + b"".join(c.docs), dtype=np.uint8), off


@functools.lru_cache(maxsize=None)
def _oracle(exprs, fold, pos_end):
    k = compiled(exprs, fold)
    o = Oracle(k.terms, POS_END if pos_end else POS_START)
    assert o.terms() == k.terms
    o.set_expression_trees(k.trees)
    return o


def matches(c):
    """the canonical match CSR of the case's documents by the oracle's scan (match_off, term_id, pos)"""
    blob, off = packed(c)
    return _oracle(c.exprs, c.fold, c.pos_end).scan(blob, off, fold=c.fold)


def true_rows(exprs, docs, fold):
    """the rows of ProcessText over the documents by the oracle, tail bits ones"""
    k = compiled(exprs, fold)
    off = np.zeros(len(docs) + 1, dtype=np.uint64)
    if docs:
        off[1:] = np.cumsum([len(d) for d in docs], dtype=np.uint64)
    blob = np.frombuffer(b"".join(docs) + b"\0", dtype=np.uint8)
    rows = _oracle(exprs, fold, False).process(blob, off, fold=fold)
    return with_tail(rows, len(k.programs))


def with_tail(words, n_exprs):
    words = np.array(words, dtype=np.uint32)
    if n_exprs & 31 and words.size:
        words[..., -1] |= np.uint32((0xFFFFFFFF << (n_exprs & 31)) & 0xFFFFFFFF)
    return words


def want_of(n_exprs, cols):
    """a mask with the bits `cols`, tail bits ones"""
    w = np.zeros((n_exprs + 31) // 32, dtype=np.uint32)
    for i in cols:
        w[i >> 5] |= np.uint32(1 << (i & 31))
    return with_tail(w, n_exprs)


def reference(c, not_is_witness=False, no_and_one=False, clear_tail=False, ignore_row_idx=False):
    """(total, span_off, start, len, term) of the contract, by plain loops over the oracle's matches.  The keyword arguments are
    the wrong readings assert_not_vacuous asks about: units under a NOT as witnesses; the bit test without its `& 1`, i.e.
    (word >> (i & 31)) != 0, which lets the bits above i speak -- the tail bits among them (clear_tail: on rows and masks whose
    tail bits are cleared first); r(d) = d whatever row_idx says (modulo the rows there are)"""
    k = compiled(c.exprs, c.fold)
    E = len(k.programs)
    sets = k.witness_sets(not_is_witness)
    moff, tid, pos = matches(c)
    rows, want = c.rows, c.want
    if clear_tail and E & 31:
        keep = np.uint32((1 << (E & 31)) - 1)
        rows = rows.copy()
        rows[:, -1] &= keep
        if want is not None:
            want = want.copy()
            want[-1] &= keep
    lists = [[i for i in range(E) if t in sets[i]] for t in range(k.n_terms)]
    lens = [len(t) for t in k.terms]
    memo = {}

    def kept(r, t):
        for i in lists[t]:
            w = int(rows[r, i >> 5]) & (0xFFFFFFFF if want is None else int(want[i >> 5]))
            if ((w >> (i & 31)) != 0) if no_and_one else ((w >> (i & 31)) & 1):
                return True
        return False
    span_off, start, length, term = [0], [], [], []
    moff, tid, pos = moff.tolist(), tid.tolist(), pos.tolist()
    for d in range(len(c.docs)):
        r = d % max(len(rows), 1) if ignore_row_idx or c.row_idx is None else int(c.row_idx[d])
        for m in range(moff[d], moff[d + 1]):
            t = tid[m]
            if (r, t) not in memo:
                memo[(r, t)] = kept(r, t)
            if memo[(r, t)]:
                start.append(pos[m] + 1 - lens[t] if c.pos_end else pos[m])
                length.append(lens[t])
                term.append(t)
        span_off.append(len(start))
    return len(start), span_off, start, length, term


def case(name, exprs, docs, rows=None, row_idx=None, want=None, pos_end=False, fold=False, lead=b"", slack=b"", at=0):
    exprs = tuple(exprs)
    docs = tuple(d.encode("utf-8") if isinstance(d, str) else bytes(d) for d in docs)
    if rows is None:
        rows = true_rows(exprs, docs, fold)
    return Case(name, exprs, docs, np.ascontiguousarray(rows, dtype=np.uint32), None if row_idx is None else np.asarray(row_idx, dtype=np.uint64),
                want, pos_end, fold, bytes(lead), bytes(slack), at)


def through(c, name, perm):
    """the case with its rows stored in another order and row_idx leading back to them: rows'[perm[d]] = rows[d]"""
    perm = np.asarray(perm, dtype=np.uint64)
    rows = np.zeros_like(c.rows)
    rows[perm.astype(np.int64)] = c.rows
    return c._replace(name=name, rows=rows, row_idx=perm)


def twice(c, name):
    """every document twice, the second copies reading the first copies' rows: repeated entries in row_idx"""
    n = len(c.docs)
    return c._replace(name=name, docs=c.docs + c.docs, row_idx=np.asarray(list(range(n)) * 2, dtype=np.uint64))


WITNESS_EXPRS = [
    ('not "a"',), ('not (not "a")',), ('"a" and not ("b" or "c")',),
    ('"a" and "b"', '"c" and not "a"'),                                 # positive in one expression, negated in another
    ('"a" or "b"', 'not "c"'),                                          # c is a witness nowhere
    ('"a" and ("b" or "a")',),                                          # the same keyword twice
    ('inord("a" and "b")', 'inord("c" and "a") or not "d"'),            # inside INORD
    ('"a" and r"b+"', 'r"c" or "d"'),                                   # an extra (regex) slot beside keywords
    tuple('"k" and "u%d"' % i for i in range(70)),                      # a keyword in 70 expressions
] + [tuple(['not "zz"'] * (n - 1) + ['"a"']) for n in (1, 32, 33, 2081)]     # the witness at the last index


@functools.lru_cache(maxsize=None)
def fixed_cases():
    T, _ = spans_shape()
    c = []
    # the witness table, on documents that hold every keyword and on some that do not
    for k, exprs in enumerate(WITNESS_EXPRS):
        kw = [t.decode() for t in compiled(exprs, False).terms]
        docs = [" ".join(kw), " ".join(reversed(kw)), "", "a", "a b", "c a", "d", "k u3 k u69", "zz a", "b c d"]
        c.append(case("witness %d: %s" % (k, exprs[-1] if len(exprs) > 3 else " | ".join(exprs)), exprs, docs))
    # mark and place: match counts at the tile's borders ("a" * k holds k matches of "a")
    ab = ('"a" and "b"', '"c"', 'not "a"')
    edge = [0, 1, T - 1, T, T + 1]
    c.append(case("match counts at the tile borders", ab, ["a" * k + "b" * (k % 2) for k in edge]))
    c.append(case("one document of 3T+5 matches", ab, ["x", "ab" * ((3 * T + 5) // 2) + "a", "c"]))
    gap = ["ab"] + ["xyz"] * 300 + ["abc"]
    c.append(case("300 documents without a match between two with", ab, gap))
    c.append(case("300 documents without a match in front", ab, ["xyz"] * 300 + ["ab", "ac"]))
    c.append(case("300 documents without a match at the end", ab, ["ab", "ca"] + [""] * 300))
    mixed = ["ab", "a", "b", "c", "abc", "", "ca", "ba" * 40, "cc", "xa"] * 7
    base = case("mixed documents, identity", ab, mixed)
    c.append(base)
    rng = np.random.default_rng(5)
    c.append(through(base, "mixed documents, rows permuted", rng.permutation(len(mixed))))
    c.append(twice(base, "mixed documents twice, repeated row indices"))
    c.append(base._replace(name="mixed documents, empty mask", want=want_of(3, [])))
    c.append(base._replace(name="mixed documents, one column", want=want_of(3, [1])))
    c.append(base._replace(name="mixed documents, every column by a mask", want=want_of(3, [0, 1, 2])))
    c.append(case("nothing is kept", ('"a" and "q"', 'not "b"'), mixed))
    c.append(case("everything is kept", ('"a" or "b" or "c"',), [d for d in mixed if d]))
    # geometry
    geo = ('"abc" or "bcd" or "abcd"', '"x"')
    for pe in (False, True):
        tag = "POS_END" if pe else "POS_START"
        c.append(case("abc, bcd and abcd in xabcdx, " + tag, geo, ["xabcdx", "abcd", "bcd", "zabc", "abcz"], pos_end=pe))
        c.append(case("a keyword at the first and at the last byte, " + tag, ('"ab"',), ["ab", "abab", "ab--ab", "-ab-", "a", "b"], pos_end=pe))
        c.append(case("upper-case text under the fold, " + tag, ('"Abc" and "dE"',), ["ABC de", "abcDE", "AbC", "xxABCDExx"], pos_end=pe, fold=True))
        c.append(case("fold-safe Latin-1 text, " + tag, ('"café" or "ÿx"',), ["Café ÿX", "CAFé", "écaféÿ", "ß"], pos_end=pe, fold=True))
        # doc_off[0] = 7 on a buffer at an odd address; the lead bytes end with, and the slack begins with, half a keyword
        c.append(case("lead bytes and slack that hold half a keyword, " + tag, geo, ["cdx abc", "abcd ab"], pos_end=pe, lead=b"bcdx ab", slack=b"cd abcd", at=1))
    # rows wider than a word, the witness at the last index
    for n in (32, 33, 2081):
        exprs = tuple(['not "zz"'] * (n - 1) + ['"a" and "b"'])
        c.append(case("%d expressions, the witness at the last index" % n, exprs, ["ab", "a", "zz ab", "b", "ba ba"]))
    return c


def _random_expr(rng, kws, depth=0):
    r = rng.random()
    if depth >= 3 or r < 0.35:
        return '"%s"' % kws[rng.integers(len(kws))]
    if r < 0.5:
        return "not (%s)" % _random_expr(rng, kws, depth + 1)
    if r < 0.58:
        return "inord(%s and %s)" % ('"%s"' % kws[rng.integers(len(kws))], '"%s"' % kws[rng.integers(len(kws))])
    return "(%s %s %s)" % (_random_expr(rng, kws, depth + 1), "and" if rng.random() < 0.5 else "or", _random_expr(rng, kws, depth + 1))


@functools.lru_cache(maxsize=None)
def random_cases():
    """seeded batches of up to 2 000 short documents over a small alphabet, true rows or random ones, every kind of row_idx and mask"""
    rng = np.random.default_rng(20241019)
    out = []
    for i, (n, n_exprs, n_kw) in enumerate([(2000, 40, 12), (1500, 33, 20), (800, 70, 8), (1200, 5, 5), (600, 64, 30), (2000, 31, 10)]):
        kws = sorted({"".join(rng.choice(list("abc"), rng.integers(1, 4))) for _ in range(n_kw)})
        exprs = tuple(_random_expr(rng, kws) for _ in range(n_exprs))
        docs = ["".join(rng.choice(list("abcd "), rng.integers(0, 60))) for _ in range(n)]
        pe = i % 2 == 1
        b = case("random %d: %d documents, %d expressions" % (i, n, n_exprs), exprs, docs, pos_end=pe, lead=b"ab" * (i % 3), at=i % 4)
        out.append(b)
        out.append(through(b, b.name + ", rows permuted", rng.permutation(n))._replace(want=want_of(n_exprs, rng.integers(0, n_exprs, 3).tolist())))
        W = (n_exprs + 31) // 32
        rnd = with_tail(rng.integers(0, 1 << 32, (n // 2, W), dtype=np.uint64).astype(np.uint32) &
                        rng.integers(0, 1 << 32, (n // 2, W), dtype=np.uint64).astype(np.uint32), n_exprs)
        out.append(b._replace(name=b.name + ", random rows through random indices", rows=rnd, row_idx=rng.integers(0, n // 2, n).astype(np.uint64)))
    return out


def all_cases():
    return fixed_cases() + random_cases()


@functools.lru_cache(maxsize=None)
def expected():
    """{name: (total, span_off, start, len, term)} of all_cases(), computed once"""
    return {c.name: reference(c) for c in all_cases()}


# ---- redaction cases ----------------------------------------------------------------------------------------------------------
# blob: random bytes, lead bytes and 64 bytes of slack included (doc_off[-1] + 64 = len(blob)); ok False: a span reaches past its document
FillCase = collections.namedtuple("FillCase", "name blob doc_off span_off start length mask ok")


def redact_reference(f, mutant=None):
    """the masked bytes, by slicing a bytearray; the spans are read at the caller's indexes, [span_off[0], span_off[n_docs]).  None:
    a span that was read reaches past its document (the call refuses).  mutant "span_at_k": the spans read at k, the index behind
    the base, instead of span_off[0] + k"""
    out = bytearray(f.blob.tobytes())
    s0 = int(f.span_off[0])
    for d in range(len(f.doc_off) - 1):
        for s in range(int(f.span_off[d]), int(f.span_off[d + 1])):
            at = s - s0 if mutant == "span_at_k" else s
            a, n = int(f.doc_off[d]) + int(f.start[at]), int(f.length[at])
            if a + n > int(f.doc_off[d + 1]):
                return None
            out[a:a + n] = bytes([f.mask]) * n
    return bytes(out)


FULL = 0xFFFFFFFF


def fill_case(name, doc_lens, spans, mask=0x2A, seed=1, lead=0, ok=True, span_lead=0, span_tail=0):
    """spans: per document a list of (start, len).  span_lead / span_tail: entries of the span arrays in front of the batch's spans
    (span_off[0] = span_lead) and behind them; they hold FULL, FULL -- a span the call would refuse if it read it"""
    rng = np.random.default_rng(seed)
    off = np.zeros(len(doc_lens) + 1, dtype=np.uint64)
    off[0] = lead
    off[1:] = lead + np.cumsum(np.asarray(doc_lens, dtype=np.uint64))
    blob = rng.integers(0, 256, int(off[-1]) + 64, dtype=np.uint8)
    blob[blob == mask] ^= 0x55                                          # (a masked byte is then one the fill wrote)
    so = np.full(len(doc_lens) + 1, span_lead, dtype=np.uint64)
    so[1:] = span_lead + np.cumsum([len(s) for s in spans], dtype=np.uint64)
    flat = [(FULL, FULL)] * span_lead + [p for s in spans for p in s] + [(FULL, FULL)] * span_tail
    return FillCase(name, blob, off, so, np.asarray([p[0] for p in flat], dtype=np.uint32), np.asarray([p[1] for p in flat], dtype=np.uint32), mask, ok)


@functools.lru_cache(maxsize=None)
def fill_cases(span_lead=0, span_tail=0):
    """the same batches -- texts, spans, names -- whatever the base: only the span arrays' placement differs"""
    _, S = spans_shape()
    big = 7424
    fill_case = functools.partial(globals()["fill_case"], span_lead=span_lead, span_tail=span_tail)
    c = [fill_case("spans of 1, 63, 64, 65 and 7 424 bytes", [9000], [[(3, 1), (10, 63), (100, 64), (200, 65), (1000, big)]], seed=2, lead=5),
         fill_case("a span of 7 424 bytes among one-byte spans", [50, big + 2, 50], [[(k, 1) for k in range(0, 50, 3)], [(1, big)], [(49, 1), (0, 1)]], seed=3),
         fill_case("overlapping, nested, identical and adjacent spans", [200],
                   [[(10, 20), (20, 20), (50, 40), (60, 5), (100, 7), (100, 7), (120, 4), (124, 4), (128, 1)]], seed=4, lead=3),
         fill_case("no spans at all", [10, 0, 30], [[], [], []], seed=5),
         fill_case("no documents with spans but empty ones between", [0, 0, 5, 0], [[], [], [(0, 5)], []], seed=6),
         fill_case("a span that ends on the document's last byte", [40, 40], [[(30, 10)], [(0, 40), (39, 1)]], seed=7, lead=1),
         fill_case("spans of length 0", [20], [[(0, 0), (5, 3), (20, 0), (8, 0)]], seed=8),
         fill_case("mask 0 and mask 255", [64], [[(1, 62)]], mask=0, seed=9),
         fill_case("mask 255", [64], [[(1, 62)]], mask=255, seed=10),
         fill_case("a span one byte too long", [40, 40, 40], [[(0, 4)], [(30, 11)], [(5, 5)]], seed=11, lead=2, ok=False),
         fill_case("a span that starts behind its document", [40, 40], [[(41, 0)], [(5, 5)]], seed=12, ok=False),
         fill_case("a span whose start plus length wraps 32 bits", [40], [[(8, 0xFFFFFFFC)]], seed=13, ok=False)]
    rng = np.random.default_rng(77)
    for n in (S - 1, S, S + 1, 3 * S + 5):
        lens = rng.integers(0, 40, n)
        c.append(fill_case("a tile of %d spans" % n, [5000], [[(int(rng.integers(0, 4900)), int(x)) for x in lens]], seed=20 + n))
        docs = rng.integers(1, 30, n).tolist()
        c.append(fill_case("%d documents of one span each" % n, docs, [[(int(rng.integers(0, L)), 1)] for L in docs], seed=40 + n, lead=n % 5))
    n = 3000
    docs = rng.integers(0, 80, n).tolist()
    spans = [[(int(a), int(rng.integers(0, L - a + 1))) for a in rng.integers(0, L + 1, rng.integers(0, 4))] if L else [] for L in docs]
    c.append(fill_case("random: 3 000 documents", docs, spans, seed=99, lead=7))
    return c


# ---- the cases are not vacuous ------------------------------------------------------------------------------------------------
def assert_not_vacuous():
    """conditions on the inputs, evaluated on the CPU: some case would answer differently if units under a NOT were witnesses, some if
    the tail bits were honoured (the bit test without `& 1` answers differently on the case's rows and masks than on the same with
    their tail bits cleared), some if row_idx were ignored; and the kept share of matches is strictly between 0 and 1 in more than
    20 cases"""
    cases = all_cases()
    exp = expected()
    nots = [c.name for c in cases if reference(c, not_is_witness=True) != exp[c.name]]
    assert nots, "no case would notice units under a NOT kept as witnesses"
    tails = [c.name for c in cases if len(c.exprs) & 31 and reference(c, no_and_one=True) != reference(c, no_and_one=True, clear_tail=True)]
    assert tails, "no case would notice a walk that honours the tail bits"
    idx = [c.name for c in cases if c.row_idx is not None and reference(c, ignore_row_idx=True) != exp[c.name]]
    assert idx, "no case would notice a walk that ignores row_idx"
    some = [c.name for c in cases if 0 < exp[c.name][0] < len(matches(c)[1])]
    assert len(some) > 20, len(some)
    assert_fill_not_vacuous()
    return nots, tails, idx, some


def assert_fill_not_vacuous(span_lead=1, span_tail=1):
    """the redaction that reads its spans at k instead of span_off[0] + k is the reference itself on every fill case handed over with
    span_off[0] == 0 -- that is the gap -- and differs (masks other bytes, or is refused over the poison in front) on some fill case
    handed over behind span_lead entries.  Returns the names of those"""
    blind = [f.name for f in fill_cases() if f.ok and redact_reference(f, "span_at_k") != redact_reference(f)]
    assert not blind, "the mutant span_at_k shows without a span base on %r" % blind
    told = [f.name for f in fill_cases(span_lead, span_tail) if f.ok and redact_reference(f, "span_at_k") != redact_reference(f)]
    assert told, "no fill case behind a span base of %d tells the mutant span_at_k from the contract" % span_lead
    return told
