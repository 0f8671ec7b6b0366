"""Random INORD trees for the solver tests (test infrastructure): a seeded generator of expression strings whose INORD groups
are arbitrary AND/OR trees, a restatement of the pair arithmetic by which gft_set_programs sorts groups into narrow / wide /
host, document builders, and the families of (dictionary, expressions, documents, caller-supplied matches) that
test_inord_trees_host.py (CPU: the product's host solver against the oracle, and the families' coverage) and
test_gpu_inord_trees.py (the device solver against the oracle) share.  Nothing here imports the product."""
import functools

import numpy as np

from helpers import OP_AND, OP_INORD, OP_NOT, OP_OR, OP_UNIT, INORD_FLAG, tree_to_program
from oracle import dsl_ref
from oracle.pyoracle import Oracle, POS_END, POS_START, pack_strings

# the device solver's limits (csrc/gft_kernels.hpp: kMaxPairs, kMaxPairDepth, kMaxPairsWide, kMaxPairDepthWide), restated
MAX_PAIRS, MAX_PAIR_DEPTH, MAX_PAIRS_WIDE, MAX_PAIR_DEPTH_WIDE = 64, 32, 8192, 64
NARROW, WIDE, HOST = "narrow", "wide", "host"


# ---- pair arithmetic ---------------------------------------------------------------------------------------------------
def group_stats(words):
    """-> ([(alive, depth)] per INORD group, deepest boolean stack of the whole program).  Inside a group a UNIT counts one
    (slot, threshold) pair, AND leaves the right operand's count, OR the sum; `alive` is the sum over the operand stack at
    its peak, `depth` the size of that stack at its peak."""
    groups, stack, sp, max_sp, alive, depth = [], [], 0, 0, 0, 0
    for w in words:
        op, fl = w >> 28, bool(w & INORD_FLAG)
        if op == OP_UNIT:
            sp += 1
            if fl:
                stack.append(1)
        elif op in (OP_AND, OP_OR):
            sp -= 1
            if fl:
                r = stack.pop()
                stack[-1] = r if op == OP_AND else stack[-1] + r
        elif op == OP_INORD:
            assert len(stack) == 1
            groups.append((alive, depth))
            stack, alive, depth = [], 0, 0
        else:
            assert op == OP_NOT and not stack
        max_sp = max(max_sp, sp)
        alive, depth = max(alive, sum(stack)), max(depth, len(stack))
    assert sp == 1 and not stack
    return groups, max_sp


def classify(words):
    """where gft_set_programs sends the expression: NARROW (a pair per lane), WIDE (compaction / scratch path) or HOST"""
    groups, max_sp = group_stats(words)
    if any(a > MAX_PAIRS_WIDE or d > MAX_PAIR_DEPTH_WIDE for a, d in groups):
        return HOST
    if any(a > MAX_PAIRS or d > MAX_PAIR_DEPTH for a, d in groups):
        return HOST if max_sp > MAX_PAIR_DEPTH_WIDE else WIDE       # (the wide evaluator's boolean stack: a bit per entry)
    return NARROW


def words_of(expr):
    """the program of an expression string with every literal on slot 0 (for the arithmetic above)"""
    return tree_to_program(dsl_ref.parse(expr, True)[0], lambda lit: 0)


# ---- expression strings ------------------------------------------------------------------------------------------------
def q(t):
    return '"%s"' % (t.decode("ascii") if isinstance(t, bytes) else t)


def flat(leaves, op):
    """leaves joined by one operator, no parentheses: the parser nests them to the left"""
    return "(%s)" % (" %s " % op).join(leaves)


def balanced(leaves, op):
    if len(leaves) == 1:
        return leaves[0]
    k = len(leaves) // 2
    return "(%s %s %s)" % (balanced(leaves[:k], op), op, balanced(leaves[k:], op))


def right_chain(leaves, op):
    e = leaves[-1]
    for t in reversed(leaves[:-1]):
        e = "(%s %s %s)" % (t, op, e)
    return e


def gen_tree(rng, leaves, p_or, shape):
    """a random AND/OR tree over `leaves` (quoted strings, in this order): shape "left" / "right" / "balanced" / "random" picks
    where every node splits its leaves"""
    n = len(leaves)
    if n == 1:
        return leaves[0]
    k = {"left": n - 1, "right": 1, "balanced": n // 2}.get(shape) or int(rng.integers(1, n))
    op = "or" if rng.random() < p_or else "and"
    return "(%s %s %s)" % (gen_tree(rng, leaves[:k], p_or, shape), op, gen_tree(rng, leaves[k:], p_or, shape))


def gen_group(rng, terms, n_leaves, p_or=0.5, shape=None):
    shape = shape or ("left", "right", "balanced", "random")[int(rng.integers(4))]
    if n_leaves > 60 and shape in ("left", "right"):            # (the parser recurses once per parenthesis)
        shape = "random"
    leaves = [q(terms[int(i)]) for i in rng.integers(0, len(terms), n_leaves)]      # terms may repeat
    return "inord(%s)" % gen_tree(rng, leaves, p_or, shape)


def gen_expr(rng, terms, n_leaves, p_or=0.5, max_groups=3):
    """1..max_groups INORD groups (each possibly under a NOT) and ordinary terms around them, joined by and / or"""
    parts = []
    for _ in range(int(rng.integers(1, max_groups + 1))):
        g = gen_group(rng, terms, int(n_leaves() if callable(n_leaves) else n_leaves), p_or)
        parts.append("not (%s)" % g if rng.integers(8) == 0 else g)
    for _ in range(int(rng.integers(0, 3))):
        t = q(terms[int(rng.integers(len(terms)))])
        parts.insert(int(rng.integers(len(parts) + 1)), "not " + t if rng.integers(3) == 0 else t)
    e = parts[0]
    for p in parts[1:]:
        e = "(%s %s %s)" % (e, "and" if rng.integers(5) else "or", p)
    return e


def without_inord(expr):
    """the same expression with every inord(X) replaced by (X): presence alone"""
    return expr.replace("inord(", "(")


# ---- documents ---------------------------------------------------------------------------------------------------------
def short_doc(rng, alphabet, max_len):
    if rng.integers(3):                                          # two documents in three: the letters thinned out once more
        alphabet = alphabet + b"." * len(alphabet)
    return bytes(alphabet[int(i)] for i in rng.integers(0, len(alphabet), int(rng.integers(0, max_len + 1))))


def planted_doc(rng, size, placements):
    """`size` bytes of filler ('.' and ' ', bytes of no term) with the terms of placements = [(offset, term)] written over
    it; an offset that would overlap an earlier placement or the end moves behind it / in front of it"""
    buf = bytearray(b". "[int(i)] for i in rng.integers(0, 2, size))
    used = []
    for at, t in placements:
        at = max(0, min(int(at), size - len(t)))
        moved = True
        while moved:
            moved = False
            for a, b in used:
                if at < b + 1 and a < at + len(t) + 1:
                    at, moved = b + 1, True
        if at + len(t) > size:
            continue
        buf[at:at + len(t)] = t
        used.append((at, at + len(t)))
    return bytes(buf)


# ---- families ----------------------------------------------------------------------------------------------------------
class Family:
    """terms: the dictionary (sorted bytes); exprs: expression strings; texts: documents; extra_lits: literals that are no
    dictionary terms, extra slot j = len(terms) + j; extra: per document [(literal, position)] in the order given to the
    solver (ascending per literal); classes: per expression NARROW / WIDE / HOST or None (not stated); named: rows
    (expression index, document index, expected truth) derived by hand"""

    def __init__(self, name, terms, exprs, texts, extra_lits=(), extra=None, classes=None, named=(), named_mode=None):
        self.name, self.terms, self.exprs, self.texts = name, sorted(set(terms)), list(exprs), list(texts)
        self.extra_lits = list(extra_lits)
        self.extra = extra if extra is not None else [[] for _ in texts]
        self.classes = classes or [None] * len(exprs)
        self.named, self.named_mode = list(named), named_mode
        assert len(self.extra) == len(self.texts) and len(self.classes) == len(self.exprs)
        self.trees = [dsl_ref.parse(e, True)[0] for e in self.exprs]
        self._ref = {}

    def slot_of(self, lit):
        b = lit.encode("ascii")
        if b in self._tid:
            return self._tid[b]
        return len(self.terms) + self.extra_lits.index(lit)

    def programs(self):
        self._tid = {t: i for i, t in enumerate(self.terms)}
        return [tree_to_program(t, self.slot_of) for t in self.trees]

    def packed(self, n_docs=None):
        return pack_strings(self.texts[:n_docs])

    def oracle(self, pos_mode):
        o = Oracle(self.terms, pos_mode)
        assert o.terms() == self.terms            # (term id == index: what slot_of relies on)
        return o

    def extra_engine(self, n_docs=None):
        """(off u64, absolute slot u32, pos u32) of gft_extra_matches, or None"""
        if not self.extra_lits:
            return None
        rows = self.extra[:n_docs]
        off = np.zeros(len(rows) + 1, np.uint64)
        off[1:] = np.cumsum([len(r) for r in rows])
        sl = [len(self.terms) + self.extra_lits.index(l) for r in rows for l, _ in r]
        po = [p for r in rows for _, p in r]
        return off, np.asarray(sl + [0], np.uint32), np.asarray(po + [0], np.uint32)

    def reference(self, pos_mode, exprs=None):
        """the oracle's bitmap over all documents [n_docs, words] (computed once per position mode)"""
        key = (pos_mode, None if exprs is None else tuple(exprs))
        if key not in self._ref:
            o = self.oracle(pos_mode)
            o.set_expressions(self.exprs if exprs is None else exprs, True)
            blob, off = self.packed()
            used = set(o.literals)
            assert all(l in used for l in self.extra_lits) or exprs is not None
            x = None
            if self.extra_lits:
                xo = np.zeros(len(self.extra) + 1, np.uint64)
                rows = [[(l, p) for l, p in r if l in used] for r in self.extra]
                xo[1:] = np.cumsum([len(r) for r in rows])
                x = (xo, np.asarray([o.literals.index(l) for r in rows for l, _ in r] + [0], np.int32),
                     np.asarray([p for r in rows for _, p in r] + [0], np.int64))
            bm = o.process(blob, off, extra=x)
            bm.setflags(write=False)
            self._ref[key] = bm
        return self._ref[key]

    def truth(self, pos_mode, exprs=None):
        bm = self.reference(pos_mode, exprs)
        n = len(self.exprs)
        return np.array([[bm[d, i >> 5] >> (i & 31) & 1 for i in range(n)] for d in range(len(self.texts))], dtype=bool)

    def coverage(self, pos_mode):
        """over the (INORD expression, document) pairs, on the oracle's bitmap alone: fraction true, fraction false, and
        among the pairs whose inord-free form is true the fraction whose INORD form is false"""
        has = np.array(["inord(" in e for e in self.exprs])
        t = self.truth(pos_mode)[:, has]
        p = self.truth(pos_mode, [without_inord(e) for e in self.exprs])[:, has]
        # (an expression with a NOT over a group can be true where its inord-free form is false: only pairs with p count)
        return t.mean(), 1.0 - t.mean(), (p & ~t).sum() / max(1, p.sum())


SHORT_ALPHABET = b"abcdef" + b"." * 8          # (sparse letters: few repeats, so the order of the occurrences decides)
SHORT_TERMS = [b"a", b"b", b"c", b"d", b"e", b"f", b"aa", b"aab", b"ab", b"abc", b"ba"]

# (expression, text, truth with start positions, truth with end positions), derived by hand from the reference's
# dsl/expression.go:66-142 (solve) and :175-189 (getLowestIdxGTVal: the first element GREATER than lpos[0])
QUIRKS = [
    # AND nested to the right (:78-93): inner = c's positions > b[0]; outer = those > a[0].  "cab": c = [0], b = [2]: none
    ('inord("a" and ("b" and "c"))', "abc", True, True),
    ('inord("a" and ("b" and "c"))', "bca", False, False),    # inner [1]; nothing in it lies behind a[0] = 2
    ('inord("a" and ("b" and "c"))', "cab", False, False),
    # inner [2] (> b[0] = 0), outer: 2 > a[0] = 1 -- although b lies in FRONT of a (the flat chain a, b, c is false here)
    ('inord("a" and ("b" and "c"))', "bac", True, True),
    ('inord("a" and "b" and "c")', "bac", False, False),
    # OR merges (:111-114, :192-225), AND compares with the FIRST element of the merged left list (:89)
    ('inord(("a" or "b") and ("b" or "a"))', "ab", True, True),     # l = r = [0 1]: 1 > 0
    ('inord(("a" or "b") and ("b" or "a"))', "a", False, False),    # l = r = [0]
    ('inord(("a" or "b") and ("b" or "a"))', "aa", True, True),
    # the same term three times needs three occurrences: a = [0 2] -> [2] -> none; a = [0 2 4] -> [2 4] -> [4]
    ('inord("a" and "a" and "a")', "a.a", False, False),
    ('inord("a" and "a" and "a")', "a.a.a", True, True),
    # overlapping occurrences count: "aaa" holds aa at 0 and 1
    ('inord("aa" and "aa")', "aa", False, False),
    ('inord("aa" and "aa")', "aaa", True, True),
    ('inord("aa" and "aa")', "aaaa", True, True),
    # equal starts, different ends: with start positions ab = [0], abc = [0]: 0 > 0 is false both ways round; with end
    # positions ab = [1], abc = [2]: abc lies behind ab, not the other way round -- the comparison is strict (:181)
    ('inord("ab" and "abc")', "abc", False, True),
    ('inord("abc" and "ab")', "abc", False, False),
    # a left operand that is an OR with an absent term: the absent key contributes no list (:69-72, :195-200)
    ('inord(("f" or "a") and "b")', "ab", True, True),
    ('inord(("f" or "a") and "b")', "ba", False, False),
    ('inord(("a" or "f") and "b")', "ab", True, True),
    ('inord(("f" or "e") and "b")', "ab", False, False),       # both absent: lval false, no positions
]


@functools.lru_cache(maxsize=None)
def family_narrow(seed=1):
    """(a) narrow groups over short documents: at most 64 pairs alive, pair depth at most 32"""
    rng = np.random.default_rng(1000 + seed)
    exprs = []
    while len(exprs) < 150:
        k = len(exprs)
        if k % 15 == 14:            # some large OR-heavy groups, up to the limit of 64 pairs
            e = gen_expr(rng, SHORT_TERMS, lambda: int(rng.integers(20, 65)), p_or=0.85, max_groups=1)
        else:
            e = gen_expr(rng, SHORT_TERMS, lambda: int(rng.integers(2, 7)), p_or=(0.15, 0.4)[k % 2], max_groups=2)
        if classify(words_of(e)) == NARROW:
            exprs.append(e)
    texts = [short_doc(rng, SHORT_ALPHABET, 40) for _ in range(130)]
    texts[0], texts[1] = b"", b"a"
    # the named rows, in front of the random ones (so every document count > 1 has some of them)
    named_texts = list(dict.fromkeys(t.encode() for _, t, _, _ in QUIRKS))
    texts = texts[:1] + named_texts + texts[1:130 - len(named_texts)]
    exprs += list(dict.fromkeys(e for e, _, _, _ in QUIRKS))
    named = [(exprs.index(e), texts.index(t.encode()), vs, ve) for e, t, vs, ve in QUIRKS]
    return Family("narrow", SHORT_TERMS, exprs, texts, classes=[NARROW] * len(exprs), named=named)


def _pool(n, rng):
    """n distinct terms: two-letter ones over q-v and three-letter ones over g-p, so that none lies inside another or across a
    separator and a document holds exactly the terms written into it"""
    out = set()
    while len(out) < min(n // 6, 30):
        out.add(bytes(b"qrstuv"[int(i)] for i in rng.integers(0, 6, 2)))
    while len(out) < n:
        out.add(bytes(b"ghijklmnop"[int(i)] for i in rng.integers(0, 10, 3)))
    out = sorted(out)
    return [out[int(i)] for i in rng.permutation(n)]


def _subset_doc(rng, terms, k):
    """k of the terms (all when k >= len) in random order"""
    k = min(k, len(terms))
    pick = [terms[int(i)] for i in rng.permutation(len(terms))[:k]]
    return b".".join(pick)


@functools.lru_cache(maxsize=None)
def family_limits():
    """(b) one pair of expressions on either side of every limit of the device solver"""
    rng = np.random.default_rng(2000)
    pool = _pool(72, rng)
    A, B = pool[:36], pool[36:]                                  # left operands draw from A, right operands from B
    qa, qb = [q(t) for t in A], [q(t) for t in B]
    exprs, classes = [], []

    def add(e, c):
        exprs.append(e)
        classes.append(c)
    # (OR of k) and (OR of m): 63 and 64 pairs alive stay on the lanes, 65 is the wide path
    add("inord(%s and %s)" % (flat(qa[:31], "or"), flat(qb[:32], "or")), NARROW)
    add("inord(%s and %s)" % (flat(qa[:32], "or"), flat(qb[:32], "or")), NARROW)
    add("inord(%s and %s)" % (flat(qa[:32], "or"), flat(qb[:33], "or")), WIDE)
    add("inord(%s and %s)" % (balanced(qa[:33], "or"), balanced(qb[:32], "or")), WIDE)
    # a chain nested to the right: a pair-stack entry per leaf
    chain = [q(pool[(7 * i) % len(pool)]) for i in range(65)]
    for n, c in ((32, NARROW), (33, WIDE), (64, WIDE), (65, HOST)):
        add("inord(%s)" % right_chain(chain[:n], "and"), c)
    # OR halves of 8 192 and 8 193 pairs alive (terms repeat)
    big_a, big_b = [qa[i % len(qa)] for i in range(4097)], [qb[(5 * i) % len(qb)] for i in range(4096)]
    add("inord(%s and %s)" % (balanced(big_a[:4096], "or"), balanced(big_b, "or")), WIDE)
    add("inord(%s and %s)" % (balanced(big_a, "or"), balanced(big_b, "or")), HOST)
    # a wide group under a boolean stack deeper than 64 entries (the PUBLIC postfix form): the host's
    wide = "inord(%s and %s)" % (flat(qa[:33], "or"), flat(qb[:33], "or"))
    add(right_chain([qa[i % 36] for i in range(66)] + [wide], "or"), HOST)
    add(right_chain([qa[i % 36] for i in range(61)] + [wide], "and"), WIDE)     # 63 deep: still the device's
    add("not (%s)" % wide, WIDE)
    texts = [b"", A[0], B[0]]
    while len(texts) < 64:
        ka, kb = [int(rng.choice([0, 1, 3, 18, 36])) for _ in range(2)]
        a, b = _subset_doc(rng, A, ka), _subset_doc(rng, B, kb)
        how = int(rng.choice([0, 1, 1, 1, 2, 3, 3]))
        if how == 0:
            texts.append(a + b"." + b)                           # every left term in front of every right term
        elif how == 1:
            texts.append(b + b"." + a)
        elif how == 2:
            texts.append(_subset_doc(rng, pool, ka + kb))
        else:                                                    # the chain's terms: in order, or with one out of order
            ch = [pool[(7 * i) % len(pool)] for i in range(int(rng.choice([32, 33, 64, 65])))]
            if rng.integers(3):
                ch[-1], ch[int(rng.integers(len(ch) - 1))] = ch[int(rng.integers(len(ch) - 1))], ch[-1]
            texts.append(b".".join(ch) + b"." + b".".join(ch[-1:]) * int(rng.integers(2)))
    return Family("limits", pool, exprs, texts, classes=classes)


def _wide_group(rng, terms, n_leaves, n_and):
    """a wide group: `n_and` ANDs near the root over OR trees of random shape (an AND-heavy tree of hundreds of leaves is
    false for every document that holds a few of them)"""
    leaves = [q(terms[int(i)]) for i in rng.integers(0, len(terms), n_leaves)]
    cuts = sorted(int(c) for c in rng.choice(np.arange(1, n_leaves), n_and, replace=False))
    blocks = [leaves[a:b] for a, b in zip([0] + cuts, cuts + [n_leaves])]
    shapes = ("balanced", "random", "left")
    parts = [gen_tree(rng, b, 1.0, shapes[int(rng.integers(3))] if len(b) <= 60 else "random") for b in blocks]
    return gen_tree(rng, parts, 0.0, ("left", "right", "random")[int(rng.integers(3))])


def _prefix(rng, terms, n_words):
    """`n_words` ordinary boolean words in front of a group: t or t or ... (2k - 1 words for k terms), then `and`"""
    k = (n_words + 1) // 2
    return " or ".join(q(terms[int(i)]) for i in rng.integers(0, len(terms), k)) if k else ""


@functools.lru_cache(maxsize=None)
def wide_material():
    """the dictionary and the wide expressions that (c), (d) and (e) share"""
    rng = np.random.default_rng(3000)
    pool = _pool(300, rng)
    never = [b"ww", b"wx", b"xw", b"xx", b"wwx", b"xxw"]         # dictionary terms that no document holds
    exprs, groups = [], []                                       # groups: the terms of each expression's wide groups
    for k in range(24):
        n_leaves = int(rng.integers(70, 401))
        sub = [pool[int(i)] for i in rng.permutation(300)[:int(rng.integers(40, 200))]]
        g = "inord(%s)" % _wide_group(rng, sub, n_leaves, int(rng.integers(1, 4)))
        while classify(words_of(g)) != WIDE:
            g = "inord(%s)" % _wide_group(rng, sub, n_leaves, int(rng.integers(1, 4)))
        pre = _prefix(rng, pool, int(rng.integers(0, 131)))
        exprs.append("%s and %s" % (pre, g) if pre else g)
        groups.append(sub)
    qn = [q(t) for t in never]
    qs = [q(t) for t in pool]
    # word 63 of the expression is an absent UNIT and its OR is word 0 of the next 64: t0 t1 OR t2 OR ... puts leaf k >= 1 at
    # word 2k - 1, so leaf 32 sits at word 63
    lv = qs[:32] + [qn[0]] + qs[33:45]
    exprs.append("inord(%s and %s)" % (flat(lv, "or"), flat(qs[50:90], "or")))
    groups.append(pool[:45] + pool[50:90])
    # ... and the same 64 words later (word 127 / word 0 of the next round of 128)
    lv = qs[:64] + [qn[1]] + qs[65:70]
    exprs.append("inord(%s and %s)" % (flat(lv, "or"), flat(qs[80:120], "or")))
    groups.append(pool[:70] + pool[80:120])
    # every left operand is empty
    exprs.append("inord((%s and %s) and %s)" % (flat(qn[:3], "or"), flat(qs[:40], "or"), flat(qs[40:80], "or")))
    groups.append(pool[:80])
    exprs.append("inord(%s and %s)" % (balanced(qn * 6, "or"), balanced(qs[:70], "or")))
    groups.append(pool[:70])
    # an empty left operand under an OR: the dummy must vanish, the other side decides
    exprs.append("inord(((%s and %s) or %s) and %s)" % (flat(qn[:2], "or"), flat(qs[:30], "or"), flat(qs[30:60], "or"), flat(qs[60:100], "or")))
    groups.append(pool[:100])
    exprs.append("inord((%s or (%s and %s)) and %s)" % (flat(qs[30:60], "or"), qn[3], flat(qs[:30], "or"), flat(qs[60:100], "or")))
    groups.append(pool[:100])
    exprs.append("inord(((%s and %s) or (%s and %s)) and %s)" % (qn[0], qs[0], flat(qs[100:140], "or"), flat(qs[1:30], "or"), flat(qs[60:100], "or")))
    groups.append(pool[:140])
    # two wide groups; a wide group next to a narrow one; NOT over a wide group
    w1 = "inord(%s and %s)" % (flat(qs[:40], "or"), balanced(qs[40:80], "or"))
    w2 = "inord(%s and %s)" % (balanced(qs[60:100], "or"), flat(qs[10:50], "or"))
    exprs += ["%s and %s" % (w1, w2), "%s or %s" % (w2, w1), '%s and inord(%s and %s)' % (w1, qs[3], qs[50]),
              'inord((%s or %s) and %s) or %s' % (qs[5], qs[6], qs[70], w2), "not (%s)" % w1, "%s and not (%s)" % (qs[2], w2)]
    groups += [pool[:100]] * 6
    # (d): the right operand of an AND holds more than 128 pairs, the left one more than 64; an AND that comes out empty mid-way
    L, M, R = pool[:70], pool[70:140], pool[140:290]
    ql, qm, qr = [q(t) for t in L], [q(t) for t in M], [q(t) for t in R]
    scratch = ["inord(%s and %s)" % (flat(ql, "or"), flat(qr, "or")),
               "inord(%s and %s)" % (balanced(ql, "or"), balanced(qr, "or")),
               "inord((%s and %s) and %s)" % (flat(ql, "or"), flat(qm, "or"), flat(qr, "or")),
               "inord(%s and (%s and %s))" % (flat(ql, "or"), flat(qm, "or"), balanced(qr, "or")),
               "inord((%s and %s) or %s) and %s" % (flat(ql, "or"), flat(qm, "or"), qn[0], qs[0]),
               "not (inord(%s and %s))" % (flat(qm, "or"), flat(qr, "or"))]
    for k in range(10):                                          # ... with OR trees of random shape, operands in every role
        a, b, c = [[ql, qm, qr][int(i)] for i in rng.permutation(3)]
        ta, tb, tc = [gen_tree(rng, [x[int(i)] for i in rng.permutation(len(x))], 1.0, "random") for x in (a, b, c)]
        scratch.append(("inord((%s and %s) and %s)", "inord(%s and (%s and %s))", "inord(%s and %s) and inord(%s and %s)")[k % 3]
                       % ((ta, tb, tc) if k % 3 < 2 else (ta, tb, tb, tc)))
    return pool, never, exprs, groups, scratch, (L, M, R)


@functools.lru_cache(maxsize=None)
def family_wide():
    """(c) wide groups over documents that hold 0-12 of a group's terms: the presence compaction keeps them on the lanes"""
    pool, never, exprs, groups, scratch, _ = wide_material()
    rng = np.random.default_rng(3100)
    texts = [b""]
    while len(texts) < 65:
        g = groups[int(rng.integers(len(groups)))]
        texts.append(_subset_doc(rng, g, int(rng.integers(0, 13))))
    ex = exprs + scratch
    return Family("wide", pool + never, ex, texts, classes=[WIDE] * len(ex))


@functools.lru_cache(maxsize=None)
def family_scratch():
    """(d) the same groups over documents that hold all of a group's terms, or between 65 and all: more than 64 pairs are
    alive after the compaction"""
    pool, never, exprs, groups, scratch, (L, M, R) = wide_material()
    rng = np.random.default_rng(3200)
    texts = []

    def shuffled(ts, k=None):
        return _subset_doc(rng, ts, len(ts) if k is None else k)
    for order in ((L, M, R), (R, M, L), (L, R, M), (M, L, R), (R, L, M), (M, R, L)):      # operand by operand, in every order
        for _ in range(3):
            texts.append(b".".join(shuffled(x) for x in order))
    for _ in range(6):                                           # ... and parts of them
        texts.append(b".".join(shuffled(x, int(rng.integers(30, len(x) + 1))) for x in (L, M, R)))
        texts.append(b".".join(shuffled(x, int(rng.integers(30, len(x) + 1))) for x in (R, L)))
    for g in groups[:24:2]:
        texts.append(shuffled(g))                                # all of a random group's terms
        texts.append(shuffled(g, int(rng.integers(min(65, len(g)), len(g) + 1))))
    texts.append(shuffled(pool))
    ex = scratch + exprs[:10]
    return Family("scratch", pool + never, ex, texts, classes=[WIDE] * len(ex))


LONG_SIZES = (30_000, 60_000, 70_000, 100_000, 300_000)
N_SCEN = 4


def _long_terms():
    """per scenario: A, B, C, G (4 bytes), a 40-byte term Z, and two terms that lie INSIDE Z: J (2 bytes, at offset 3) and I
    (4 bytes, at offset 5) -- letters only, nothing else inside anything else"""
    out = []
    for k in range(N_SCEN):
        c = bytes([ord("B") + k]) * 2
        J, I = b"j" + c[:1], b"I" + c + b"i"
        out.append((b"A" + c + b"x", b"A" + c + b"y", b"A" + c + b"z", b"G" + c + b"g", b"Z" + c + J + I + b"M" * 31, J, I))
    return out


@functools.lru_cache(maxsize=None)
def family_long():
    """(e) long documents: the slice walk of documents of 8 units and more, and the strided layout below that"""
    rng = np.random.default_rng(4000)
    scen = _long_terms()
    pool = _pool(100, rng)
    L, R = pool[:40], pool[40:80]
    ql, qr = [q(t) for t in L], [q(t) for t in R]
    exprs = []
    for A, B, C, G, Z, J, I in scen:
        exprs += ["inord(%s and %s)" % (q(A), q(B)), "inord(%s and %s and %s)" % (q(A), q(B), q(C)),
                  "inord((%s or %s) and (%s or %s))" % (q(A), q(G), q(B), q(C)),
                  "inord(%s and (%s or %s))" % (q(B), q(A), q(C)),
                  # Z starts in front of I and J but ends behind them: which of Z and I is the first one decides about J
                  "inord((%s or %s) and %s)" % (q(Z), q(I), q(J)),
                  "inord(%s and (%s or %s) and %s)" % (q(G), q(I), q(Z), q(J)),
                  "inord(%s and %s)" % (q(G), q(Z))]
    n_narrow = len(exprs)
    exprs += ["inord(%s and %s)" % (flat(ql, "or"), flat(qr, "or")),
              "inord(%s and %s)" % (balanced(qr, "or"), balanced(ql, "or")),
              "inord((%s and %s) and %s)" % (flat(ql[:20], "or"), flat(qr, "or"), flat(ql[20:], "or"))]
    texts = []
    for size in LONG_SIZES:
        for j in range(8):
            pl = []
            for k, (A, B, C, G, Z, J, I) in enumerate(scen):
                p = int(rng.integers(0, max(1, size // 8)))
                how = (j + k + int(rng.integers(2))) % 6
                if how == 0:                                     # successor in the same unit as the threshold
                    pl += [(p, A), (p + 50, B), (p + 120, C)]
                elif how == 1:                                   # in the next unit
                    pl += [(p, A), (p + 9000, B), (p + 18500, C)]
                elif how == 2:                                   # five units and more on
                    pl += [(p, A), (min(p + 45000, size - 300), B), (size - 100, C)]
                elif how == 3:                                   # no successor: B and C only in front of A
                    pl += [(p + 300, A), (p, B), (p + 100, C)]
                elif how == 4:                                   # B on both sides of A, C at the very end
                    pl += [(p + 12000, A), (p + 10, B), (size - 60, C), (size // 2, B)]
                else:                                            # B in front only, C behind
                    pl += [(p + 9000, A), (p, B), (p + 9100, C)]
                # Z once per document, laid over the end of a step of four slices (the slice size is the kernel's choice: the
                # two guesses are ceil(size / n) for n = ceil(size / 8 192) and one unit less), jittered; G four slices in
                # front of it.  Z then STARTS in the slice in front of that border and ENDS behind it, I and J inside it lie
                # wholly in front of the border.  Some documents have J once more further on.
                n = max(1, -(-size // 8192) - int(rng.integers(0, 2)))
                per = -(-size // n)
                step = int(rng.integers(1, max(2, n // 4 + 1)))
                edge = min(4 * step * per, size - 100)
                z_at = edge - 30 + int(rng.integers(-8, 9))
                pl += [(z_at, Z), ((4 * step - 4) * per + int(rng.integers(0, per - 100)), G)]
                if rng.integers(4) == 0:
                    pl.append((min(z_at + 5000, size - 10), J))
            # the wide groups: a few of their terms (compacted) or all of them (scratch), spread over the whole document
            if j % 4 == 2:                                       # every L term in front of every R term
                ws = list(L) + list(R)
                pl += [(int(size * (0.05 + 0.9 * i / len(ws))), t) for i, t in enumerate(ws)]
            else:
                ws = [pool[int(i)] for i in (rng.permutation(80) if j % 4 == 3 else rng.permutation(100)[:int(rng.integers(0, 13))])]
                pl += [(int(rng.integers(0, size - 10)), t) for t in ws]
            texts.append(planted_doc(rng, size, pl))
    fam = Family("long", [t for s in scen for t in s] + pool, exprs, texts)
    fam.n_narrow = n_narrow
    return fam


@functools.lru_cache(maxsize=None)
def family_extra():
    """(f) caller-supplied matches inside groups: extra literals (no dictionary terms, ascending lists) next to dictionary
    terms under OR and AND, narrow and wide; short documents and two long ones"""
    rng = np.random.default_rng(5000)
    xl = ["X%d" % i for i in range(6)]
    leaves = SHORT_TERMS + [x.encode() for x in xl] * 2
    named_e = ['inord("a" and "X0")', 'inord("X0" and "a")', 'inord(("X1" or "a") and "b")', 'inord("b" and ("X1" or "X2"))']
    exprs = list(named_e)
    while len(exprs) < 70:
        e = gen_expr(rng, leaves, lambda: int(rng.integers(2, 8)), p_or=(0.15, 0.4)[len(exprs) % 2], max_groups=2)
        if classify(words_of(e)) == NARROW and "X" in e:
            exprs.append(e)
    classes = [NARROW] * len(exprs)
    ql = [q(t) for t in leaves]
    for k in range(6):
        lv = [ql[int(i)] for i in rng.integers(0, len(ql), 120)]
        exprs.append("inord((%s and %s) and %s)" % (gen_tree(rng, lv[:40], 1.0, "random"), gen_tree(rng, lv[40:80], 1.0, "random"),
                                                      gen_tree(rng, lv[80:], 0.97, "random")))
        classes.append(WIDE)
    for x in xl:                                                 # (every extra literal is in some expression)
        exprs.append('inord(%s and "c")' % q(x))
        classes.append(NARROW)
    texts = [b"ba", b"ba", b"ab", b"ab", b"ab"]
    extra = [[("X0", 2)],                                        # the caller's match is the only successor
             [("X0", 1)],                                        # ... at the position of the dictionary match: not behind it
             [],                                                 # X1 absent from the map
             [("X1", 5), ("X2", 0)], [("X2", 0), ("X2", 1)]]
    named = [(0, 0, True, True), (0, 1, False, False), (1, 1, False, False), (2, 2, True, True),
             (3, 3, True, True), (3, 4, False, False)]
    while len(texts) < 64:
        t = short_doc(rng, SHORT_ALPHABET, 40)
        texts.append(t)
        row = []
        for x in xl:
            if rng.integers(5) < 2:
                row += [(x, int(p)) for p in sorted(rng.integers(0, len(t) + 4, int(rng.integers(1, 3))).tolist())]
        extra.append(row)
    for size in (70_000, 100_000):
        pl = [(int(rng.integers(0, size - 5)), SHORT_TERMS[int(rng.integers(len(SHORT_TERMS)))]) for _ in range(60)]
        texts.append(planted_doc(rng, size, pl))
        row = []
        for x in xl[:5]:
            row += [(x, int(p)) for p in sorted(rng.integers(0, size, int(rng.integers(1, 5))).tolist())]
        extra.append(row)
    return Family("extra", SHORT_TERMS, exprs, texts, extra_lits=xl, extra=extra, classes=classes, named=named)


FAMILIES = {"narrow": family_narrow, "limits": family_limits, "wide": family_wide, "scratch": family_scratch,
            "long": family_long, "extra": family_extra}
POS_MODES = (POS_START, POS_END)
