"""Excerpts snapped to word or line borders (gft_excerpt_spans_snap_device): the reference, written from the contract in
include/gft.h alone -- the two walks statement by statement over a `bytes`, with the decoders and the class dictionary of
word_cases.py, so nothing depends on the interpreter's Unicode version --, the fixed cases, the seeded random batches and
assert_not_vacuous(): the mutants of the reference that the fixed cases must tell apart.  Built on excerpts.py: a Case is an
excerpts.Case with a snap and a reach, expected() is excerpts.expected() with the window function replaced.  No tests in here and
none of the code under test: tests/test_excerpt_snap_host.py and tests/test_gpu_excerpt_snap.py use it."""
import functools
import random

import excerpts as X
import word_cases as W

RUNES, WORDS, LINES = 1, 2, 4
REACH_MAX = 4096
FULL = X.FULL
NL = 0x0A

# the classes: word_cases' dictionary, and the lower-case forms of its letters that the finder tests' lowered lines hold
CLASS = dict(W.CLASS)
CLASS.update({ord(c): True for c in "жà"})

_plain_window = X.window


class Case(X.Case):
    """an excerpts.Case with snap (None, "words", "lines") and reach"""

    def __init__(self, name, docs, spans, before, after, snap, reach, runes=False, lead=0):
        super().__init__(name, docs, spans, before, after, runes, lead)
        self.snap, self.reach = snap, reach

    def but(self, name, **kw):
        c = Case(name, self.docs, self.spans, self.before, self.after, self.snap, self.reach, self.runes, self.lead)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    @property
    def flags(self):
        return (RUNES if self.runes else 0) | {None: 0, "words": WORDS, "lines": LINES}[self.snap]


# ---- the contract ---------------------------------------------------------------------------------------------------------------
def is_word(rune_size, ascii_only=False):
    r, size = rune_size
    if size == 0 or r == W.RUNE_ERROR:
        return False
    if ascii_only and r >= 0x80:
        return False
    return CLASS[r]                                                 # (a KeyError: a case left the alphabet)


def last_rune(D, p):
    """utf8.DecodeLastRune(D[:p]): the decoder looks at UTFMax bytes of its slice at most, so no more is cut out"""
    return W.decode_last_rune(D[max(0, p - W.UTF_MAX):p])


def first_rune(D, p):
    """utf8.DecodeRune(D[p:]), likewise"""
    return W.decode_rune(D[p:p + W.UTF_MAX])


def cuts_word(D, p, ascii_only=False):
    return 0 < p < len(D) and is_word(last_rune(D, p), ascii_only) and is_word(first_rune(D, p), ascii_only)


def _gives_up(far, steps, reach, mutant):
    if mutant == "reach_in_runes":
        far = steps
    return far > (reach + 1 if mutant == "reach_off_by_one" else reach)


def word_start(D, lo, reach, mutant=None):
    p, steps, a = lo, 0, mutant == "ascii_class"
    while cuts_word(D, p, a):
        r = last_rune(D, p)[1]
        steps += 1
        if _gives_up(lo - (p - r), steps, reach, mutant):
            return p if mutant == "extend" else lo
        p -= r
    return p


def word_end(D, hi, reach, mutant=None):
    p, steps, a = hi, 0, mutant == "ascii_class"
    while cuts_word(D, p, a):
        r = first_rune(D, p)[1]
        steps += 1
        if _gives_up((p + r) - hi, steps, reach, mutant):
            return p if mutant == "extend" else hi
        p += r
    return p


def line_start(D, lo, reach, mutant=None):
    p, steps = lo, 0
    while p > 0 and D[p - 1] != NL:
        steps += 1
        if _gives_up(lo - (p - 1), steps, reach, mutant):
            return p if mutant == "extend" else lo
        p -= 1
    return p


def line_end(D, hi, reach, mutant=None):
    p, steps = hi, 0
    while p < len(D) and D[p] != NL:
        steps += 1
        if _gives_up((p + 1) - hi, steps, reach, mutant):
            return p if mutant == "extend" else hi
        p += 1
    if mutant == "newline_included" and p < len(D) and D[p] == NL:
        p += 1
    return p


def rune_snap(D, lo, hi):
    L = len(D)
    for _ in range(3):
        if not (0 < lo < L and D[lo] & 0xC0 == 0x80):
            break
        lo -= 1
    for _ in range(3):
        if not (hi < L and D[hi] & 0xC0 == 0x80):
            break
        hi += 1
    return lo, hi


def snap_edges(D, lo, hi, flags, reach, mutant=None):
    """the clipped window [lo, hi) of the document D -> the snapped window: what gft_debug_excerpt_snap_edges answers"""
    if flags & RUNES or (flags & WORDS and mutant != "no_implied_runes"):
        lo, hi = rune_snap(D, lo, hi)
    if flags & WORDS:
        return word_start(D, lo, reach, mutant), word_end(D, hi, reach, mutant)
    if flags & LINES:
        return line_start(D, lo, reach, mutant), line_end(D, hi, reach, mutant)
    return lo, hi


def all_edges(D, flags, reach):
    """snap_edges(D, p, p, flags, reach) for every p in [0, len(D)] -> (starts, ends), in time linear in len(D).  A walk leaves
    its edge for the first position down (up) its chain of steps that stops it, and gives up exactly when that position lies
    more than `reach` away -- the distances along the chain only grow.  test_excerpt_snap_host.py holds this against the walks
    themselves at every position of every short document"""
    L = len(D)
    down, up = list(range(L + 1)), list(range(L + 1))
    if flags & WORDS:
        cut = [cuts_word(D, p) for p in range(L + 1)]
        for p in range(L + 1):
            if cut[p]:
                down[p] = down[p - last_rune(D, p)[1]]
        for p in range(L, -1, -1):
            if cut[p]:
                up[p] = up[p + first_rune(D, p)[1]]
    elif flags & LINES:
        for p in range(1, L + 1):
            if D[p - 1] != NL:
                down[p] = down[p - 1]
        for p in range(L - 1, -1, -1):
            if D[p] != NL:
                up[p] = up[p + 1]
    starts, ends = [], []
    for p in range(L + 1):
        lo, hi = rune_snap(D, p, p) if flags & (RUNES | WORDS) else (p, p)
        starts.append(down[lo] if lo - down[lo] <= reach else lo)
        ends.append(up[hi] if up[hi] - hi <= reach else hi)
    return starts, ends


LEAD_BYTE = b"a"                                                    # what the blob mutant finds in front of the first document


def expected(case, mutant=None, span_lead=0, span_tail=0):
    """excerpts.expected() under the snapped window"""
    text = LEAD_BYTE * case.lead + b"".join(case.docs) + LEAD_BYTE * 8

    def window(doc, start, length, before, after, runes, _text=None, base=0):
        lo, hi = _plain_window(doc, start, length, before, after, False)
        if mutant == "blob":                                        # the walks see the whole blob: the lead, the neighbours, the slack
            lo, hi = snap_edges(text, base + lo, base + hi, case.flags, case.reach)
            return lo - base, hi - base
        return snap_edges(doc, lo, hi, case.flags, case.reach, mutant)
    X.window = window
    try:
        return X.expected(case, None, span_lead, span_tail)
    finally:
        X.window = _plain_window


# ---- the fixed cases ------------------------------------------------------------------------------------------------------------
def _u(s):
    return s.encode()


def neighbour_docs():
    """every pair of neighbour kinds, twice in a document: round a window's start and round its end"""
    docs, spans = [], []
    for _, a in W.NEIGHBOURS:
        for _, b in W.NEIGHBOURS:
            pre = b"ab " + a + b
            docs.append(pre + b"-+-" + a + b + b" ab")
            spans.append([(len(pre), 3)])
    return docs, spans


@functools.lru_cache(maxsize=None)
def fixed_cases(tile):
    T = tile
    cases = []
    docs, spans = neighbour_docs()
    for k in (1, 2, 3, 4):      # the start k bytes in front of the hit, the end k behind it: between the two neighbours, or inside one
        cases.append(Case("neighbours, words, %d out" % k, docs, spans, k, k, "words", 64))
    for k in (1, 2):
        cases.append(Case("neighbours, lines, %d out" % k, docs, spans, k, k, "lines", 64))
    # reach: a word that begins exactly reach and reach + 1 bytes from the edge, on both sides
    R = 5
    grown = [b". " + b"a" * n + b"hit" + b"b" * n + b" ." for n in (R - 1, R, R + 1, R + 2)]
    at_reach = Case("reach and reach + 1, words", grown, [[(2 + n, 3)] for n in (R - 1, R, R + 1, R + 2)], 0, 0, "words", R)
    cases.append(at_reach)
    # ... a two-byte rune: R runes but R + 1 bytes away, and R - 1 runes that are R bytes
    e = _u("é")
    two = [b". " + e + b"a" * (R - 1) + b"hit" + b"b" * (R - 1) + e + b" .", b". " + e + b"a" * (R - 2) + b"hit" + b"b" * (R - 2) + e + b" ."]
    cases.append(Case("a two-byte rune in the reach", two, [[(2 + 2 + R - 1, 3)], [(2 + 2 + R - 2, 3)]], 0, 0, "words", R))
    cases.append(at_reach.but("reach 0, words", reach=0))
    cases.append(at_reach.but("reach 0, words, runes given", reach=0, runes=True))
    for W_ in (REACH_MAX + 1, REACH_MAX + 2):       # the last byte of a word of W_ bytes is W_ - 1 bytes from its start
        cases.append(Case("reach 4096, a word %d bytes away" % (W_ - 1), [b" " + b"a" * W_ + b" "], [[(1, 1), (W_, 1)]], 0, 0, "words", REACH_MAX))
    long_line = b"x" * 20 + b"HIT" + b"yy\nzz"
    cases.append(Case("a line longer than the reach on one side", [long_line, long_line[::-1]], [[(20, 3)], [(len(long_line) - 23, 3)]], 0, 0, "lines", R))
    cases.append(Case("reach and reach + 1, lines", [b"\n" + b"a" * n + b"hit" + b"b" * n + b"\n" for n in (R - 1, R, R + 1)],
                      [[(1 + n, 3)] for n in (R - 1, R, R + 1)], 0, 0, "lines", R))
    cases.append(cases[-1].but("reach 0, lines", reach=0))
    # document borders: the words go on in the lead bytes, in the next document and in the slack (the tests fill both with 'a')
    cases.append(Case("words that go on outside", [b"abc", b"def ghi", b"jkl", b"", b"mno"], [[(1, 1)], [(0, 1), (6, 1)], [(1, 1)], [(0, 0)], [(0, 3)]],
                      0, 0, "words", 64, lead=3))
    cases.append(Case("lines that go on outside", [b"abc", b"def\nghi", b"jkl", b"", b"mno"], [[(1, 1)], [(0, 1), (6, 1)], [(1, 1)], [(0, 0)], [(0, 3)]],
                      0, 0, "lines", 64, lead=3))
    z = _u("中")
    cases.append(Case("a rune cut by the document's end", [b"ab" + e[:1], e[1:] + b"ab", b"ab" + z[:2], z[2:] + b"ab", z[:1] + b"ab" + z[:1]],
                      [[(1, 1)], [(1, 1)], [(0, 1)], [(2, 1)], [(1, 2)]], 0, 0, "words", 64, lead=1))
    cases.append(Case("windows at 0 and at L", [b"hello world", b"hello world", b""], [[(0, 2), (9, 2)], [(3, 1)], []], FULL, FULL, "words", 64))
    cases.append(Case("windows at 0 and at L, lines", [b"hello\nworld", b"hello\nworld"], [[(0, 2), (9, 2)], [(3, 1)]], FULL, FULL, "lines", 64))
    # merges
    cases.append(Case("one byte apart, touching after the snap", [b"xx abcdefg yy"], [[(3, 3), (7, 3)]], 0, 0, "words", 64))
    cases.append(Case("one word apart", [b"abc de fgh"], [[(0, 3), (7, 3)]], 0, 0, "words", 64))
    cases.append(Case("a span of no bytes", [b"hello world", b"hello world", b"hello\nworld"], [[(2, 0)], [(5, 0)], [(6, 0)]], 0, 0, "words", 64))
    cases.append(cases[-1].but("a span of no bytes, lines", snap="lines"))
    # the implied rune snap: an edge inside a rune of a word
    runed = _u("a\u00e9\u4e2d\U0001d49cb \u2014\U0001f600 \u00dfb\u00bd.")
    every = [[(i, 1)] for i in range(len(runed))]
    cases.append(Case("words, runes not given", [runed] * len(runed), every, 1, 1, "words", 64, runes=False))
    cases.append(cases[-1].but("words, runes given", runes=True))
    cases.append(cases[-1].but("lines, runes not given", snap="lines", runes=False))
    cases.append(cases[-1].but("lines, runes given", snap="lines", runes=True))
    # lines
    cases.append(Case("newlines at 0 and at L - 1", [b"\nfoo bar\n", b"\n", b"\n\n"], [[(5, 3)], [(0, 0), (0, 1), (1, 0)], [(1, 0)]], 0, 0, "lines", 64))
    cases.append(Case("two newlines", [b"ab\n\ncd"], [[(0, 1), (3, 0), (4, 1)]], 0, 0, "lines", 64))
    cases.append(Case("hi on a newline, lo behind one", [b"abc\ndef", b"abc\ndef"], [[(1, 2)], [(4, 1)]], 0, 0, "lines", 64))
    cases.append(Case("no newline at all", [b"abcdef", b"a\rb\rc"], [[(2, 1)], [(2, 1)]], 0, 0, "lines", 64))
    record = b"09:00 start\n09:01 ERROR disk full\n09:02 retry\n09:03 ERROR again\n09:04 ERROR thrice\nend"
    hits = [(record.find(b"ERROR"), 5), (record.find(b"disk"), 4), (record.find(b"ERROR again"), 5), (record.find(b"ERROR thrice"), 5)]
    cases.append(Case("exactly the hit lines, adjacent lines apart", [record, b"", record], [hits, [], hits[2:]], 0, 0, "lines", REACH_MAX))
    cases.append(cases[-1].but("the hit lines and a window", before=3, after=9))
    # the window pass's tiles
    for n in (T - 1, T, T + 1, 2 * T + 1):
        cases.append(Case("%d spans, words" % n, [b"abcde " * n], [[(6 * i + 2, 1) for i in range(n)]], 0, 0, "words", 64))
    n = 2 * T + 1
    cases.append(Case("%d spans, lines, documents across the tiles" % n, [b"abcde\n" * (n // 3), b"abcde\n" * (n - n // 3)],
                      [[(6 * i + 2, 1) for i in range(n // 3)], [(6 * i + 2, 1) for i in range(n - n // 3)]], 0, 0, "lines", 64, lead=5))
    return tuple(cases)


def small(cases):
    return [c for c in cases if sum(map(len, c.docs)) < 20000]


@functools.lru_cache(maxsize=None)
def random_cases(n_docs=2000, max_symbols=40, seed=20261021):
    """two seeded batches of n_docs documents of at most max_symbols symbols of word_cases.SYMBOLS: one per snap"""
    out = []
    for snap, reach, before, after, runes in (("words", 3, 2, 3, False), ("lines", 5, 1, 2, True)):
        rng = random.Random(seed + len(out))
        docs, spans = [], []
        for _ in range(n_docs):
            doc = b"".join(rng.choice(W.SYMBOLS) for _ in range(rng.randint(0, max_symbols)))
            ends = sorted(rng.randint(0, len(doc)) for _ in range(rng.randint(0, 5)))
            s = []
            for e in ends:
                n = rng.randint(0, min(e, 6))
                s.append((e - n, n))
            docs.append(doc)
            spans.append(s)
        out.append(Case("random %d, %s" % (n_docs, snap), docs, spans, before, after, snap, reach, runes, lead=3))
    return tuple(out)


MUTANTS = ("reach_off_by_one", "reach_in_runes", "blob", "extend", "ascii_class", "newline_included", "no_implied_runes")


def assert_not_vacuous(tile):
    """every mutant of the reference differs from the reference on some fixed case.  Returns {mutant: the cases that catch it}"""
    told = {}
    for m in MUTANTS:
        told[m] = [c.name for c in small(fixed_cases(tile)) if _differs(c, m)]
        assert told[m], "no fixed case tells the mutant %r from the contract" % m
    return told


def _differs(case, mutant):
    try:
        got = expected(case, mutant)
    except (AssertionError, IndexError):                            # (the mutant breaks the reference's own premises: it differs)
        return True
    want = expected(case)
    return any(got[k] != want[k] for k in want)
