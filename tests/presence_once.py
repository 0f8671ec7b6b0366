"""What k_scan5 writes to the match pool when nothing reads positions (no INORD group, no CSR): a model on the host, and the
dictionary, expressions and documents of tests/test_gpu_presence_once.py.  Needs no GPU.

The kernel writes one pool entry per match, except that the terms of a short-term record -- the terms of one to three bytes
that end at one 3-window -- are written once per work unit for all the windows that end at document offsets >= 3.  A record
is its set of terms (scan2_tables.cpp numbers the records by content), so per unit the entries are

    the matches of terms of four bytes and more
  + the matches of shorter terms that end at offsets 0, 1, 2 of the document
  + over the distinct sets of shorter terms that end together at some offset >= 3 of the unit: the size of the set.

A match belongs to the unit its END offset lies in; a document of n bytes is cut into k = ceil(n / unit_max) equal slices
(unit_slice of csrc/gft_kernels.hpp)."""
from oracle.pyoracle import POS_END, Oracle

SHORT_MAX = 3                       # bytes of the longest term a short-term record holds
START_RULE = 3                      # end offsets below this are emitted match by match


def unit_bytes(n, unit_max):
    """bytes per work unit of a document of n bytes"""
    k = 1 if n <= unit_max else (n + unit_max - 1) // unit_max
    return min((n + k - 1) // k, unit_max) if n else 1


def entries_of_matches(doc_len, matches, term_len, unit_max):
    """matches: [(term id, END offset)] of one document -> pool entries of a presence-only scan"""
    per = unit_bytes(doc_len, unit_max)
    total = 0
    sets = {}                                            # (unit, end offset) -> short terms that end there
    for t, p in matches:
        if term_len[t] > SHORT_MAX or p < START_RULE:
            total += 1
        else:
            sets.setdefault((p // per, p), set()).add(t)
    once = {(u, frozenset(s)) for (u, _), s in sets.items()}
    return total + sum(len(s) for _, s in once)


class Model:
    """the oracle's end-position scan of a dictionary -> entries per batch"""

    def __init__(self, terms):
        self.oracle = Oracle(terms, POS_END)
        self.term_len = [len(t) for t in self.oracle.terms()]

    def per_doc(self, blob, off, unit_max, fold=False):
        mo, ti, po = self.oracle.scan(blob, off, fold=fold)
        out = []
        for d in range(len(off) - 1):
            lo, hi = int(mo[d]), int(mo[d + 1])
            out.append(entries_of_matches(int(off[d + 1] - off[d]), list(zip(ti[lo:hi].tolist(), po[lo:hi].tolist())), self.term_len, unit_max))
        return out, int(ti.size)

    def entries(self, blob, off, unit_max, fold=False):
        """-> (pool entries of a presence-only scan, matches = entries of a scan with positions)"""
        per_doc, matches = self.per_doc(blob, off, unit_max, fold)
        return sum(per_doc), matches


# ---- the dictionary: 3-windows that end in "ab" carry the sets {cab, ab, b}, {xab, ab, b} and {ab, b}; "b" and "ab" sit in
# several sets; "de" shares no set with them.  The long terms stay inside a-h and x (a direct short-term table, one kernel
# instantiation); the four rotations of "abcd" make a text of "abcd..." one long match per byte ------------------------------
SHORT_TERMS = [b"b", b"ab", b"cab", b"xab", b"de"]
LONG_TERMS = [b"abcd", b"abcde", b"bcda", b"cdab", b"dabc"] + [
    b"efgh", b"fghe", b"ghef", b"hefg", b"aceg", b"bdfh", b"hgfe", b"gfeh", b"eeff", b"ffgg", b"gghh", b"hhaa",
    b"acegx", b"xgeca", b"fhfhf", b"gagag", b"hchch", b"efefe", b"axaxa", b"xhxhx",
    b"aceghf", b"hfgeca", b"ghghgh", b"fefefe", b"cfcfcf", b"xgxgxg", b"hahaha"]
TERMS = SHORT_TERMS + LONG_TERMS
FILLER = b"hhgf"                    # holds no term and no byte of a short one (with an "e" behind it: hgfe)


def lit(t):
    return '"%s"' % t.decode()


def expressions(inord=False):
    """every term on its own, NOT of every short term, ANDs and ORs across short and long terms; inord: one INORD group more"""
    ex = [lit(t) for t in TERMS] + ["not " + lit(t) for t in SHORT_TERMS]
    ex += ['"ab" and "abcd"', '"cab" or "efgh"', '"xab" and not "cab"', '"de" and ("b" or "hgfe")', '"b" and not "ab"',
           '("cab" and "xab") or "abcde"', 'not "de" and not "abcd"', '"ab" and "de" and "bcda"']
    if inord:
        ex.append('inord("ab" and "cab")')
    return ex


def fill(n):
    return (FILLER * (n // len(FILLER) + 1))[:n]


def repeats(term, n, gap=4):
    """`term` n times with filler between, behind four bytes of filler (no occurrence ends at an offset < 3)"""
    return fill(4) + (term + fill(gap)) * n


def single_unit_cases(fifo_cap):
    """name -> document of at most 8 192 bytes (one unit on an engine that has learnt nothing)"""
    many = max(200, fifo_cap // 2 + 72)                 # parked jobs beyond half the fifo: park_short drains early
    over = fifo_cap + 64                                # long matches beyond the fifo: the unit is walked again
    c = {
        "empty": b"",
        "no_short_term": fill(64) + b"efgh" + fill(9) + b"aceghf",
        "b_alone": b"b",
        "ab_alone": b"ab",
        "ab_then_cab": b"ab" + fill(12) + b"cab" + fill(5),
        "cab_then_ab": b"cab" + fill(12) + b"ab" + fill(5),
        "ab_at_start_then_ab": b"ab" + fill(8) + b"ab" + fill(8) + b"ab",
        "three_sets": fill(4) + b"cab" + fill(4) + b"xab" + fill(4) + b"hab" + fill(4) + b"de" + fill(3) + b"xab" + b"cab",
    }
    # "abcd" through an 8 000-byte unit (a long match per byte), a short term behind every `over` bytes of it
    walk, i = b"", 0
    while len(walk) < 8000:
        walk += (b"abcd" * (over // 4 + 1))[:over] + fill(4) + (b"xab", b"de", b"cab")[i % 3] + fill(5)
        i += 1
    c["second_walk"] = walk[:8000]
    for term in (b"ab", b"cab", b"de"):
        for n in (1, 2, 65, many):
            c["%s_x%d" % (term.decode(), n)] = repeats(term, n)
    assert all(len(d) <= 8192 for d in c.values()) and len(c["second_walk"]) == 8000
    return c


LONG_DOC = 20000                    # bytes: three units at 8 192, forty at 512


def long_doc(where):
    """one 20 000-byte document with short terms in its first unit, its last unit, or all through it"""
    body = bytearray(fill(LONG_DOC))
    spots = {"first": [40, 200], "last": [LONG_DOC - 300, LONG_DOC - 20], "all": list(range(100, LONG_DOC - 8, 250))}[where]
    for i, s in enumerate(spots):
        w = (b"cab", b"xab", b"de", b"ab")[i % 4] if where == "all" else b"cab"
        body[s:s + len(w)] = w
    return bytes(body)


DENSE = b"abcd" * 1024              # one long match per byte: the next call of the handle runs at 512-byte units
