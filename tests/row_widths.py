"""Rows of every width the walk over a hit bitmap treats differently, for the three calls that join a value over a row (select,
context, route; test_row_widths_host.py: the host walks, test_gpu_row_widths.py: the kernels).  W words per row: every segment width
1 << lg of the W <= 64 path with and without idle lanes, both sides of the 64-word border, rows of two and three steps.  n_cols =
32 * W - 3, so every width has a tail, and the tail bits are ones in every row and every mask.  197 documents: no rows-per-wave
value divides that, the last group of rows is always partial.  Document d carries its deciding bit in word d mod W -- in the last
word, the last valid bit -- so every word position decides some document's verdict.  The expected values are the references of
select_docs.py, context_docs.py and route_docs.py.  No tests in here."""
import collections
import functools

import numpy as np

import context_docs as CX
import route_docs as R
import select_docs as S

WIDTHS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64, 65, 66, 128, 129)
N_DOCS = 197
TAIL = np.uint32(0xE0000000)                    # the three bits at and above n_cols in a row's last word

SelectCase = collections.namedtuple("SelectCase", "name W blob doc_off rows n_cols want mode flags cols")
RouteCase = collections.namedtuple("RouteCase", "name W blob doc_off rows n_cols masks mode rest cols")


def n_cols_of(W):
    return 32 * W - 3


def _set(rows, d, col, on):
    bit = np.uint32(1 << (col & 31))
    if on:
        rows[d, col >> 5] |= bit
    else:
        rows[d, col >> 5] &= ~bit


def _batch(rng):
    lens = rng.integers(0, 41, N_DOCS)
    off = np.zeros(N_DOCS + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    return rng.integers(0, 256, int(off[-1]), dtype=np.uint8), off


def _random_rows(rng, W, keep_clear):
    """rows at a density of 30 %, the columns of keep_clear cleared, the tail bits ones"""
    rows = (rng.integers(0, 1 << 32, (N_DOCS, W), dtype=np.uint64).astype(np.uint32)
            & rng.integers(0, 1 << 32, (N_DOCS, W), dtype=np.uint64).astype(np.uint32)).astype(np.uint32)
    for c in keep_clear:
        rows[:, c >> 5] &= ~np.uint32(1 << (c & 31))
    rows[:, W - 1] |= TAIL
    return rows


def wanted_columns(W):
    """one wanted column per word; in the last word the last valid bit"""
    return [32 * j + (7 * j + 3) % 29 for j in range(W - 1)] + [n_cols_of(W) - 1]


def select_case(W, mode, flags):
    """`want` holds one column per word.  any / none: a document has at most one of them, the one of word d mod W, and has it iff its
    flag is set.  all: a document has all of them but, iff its flag is set, the one of word d mod W"""
    rng = np.random.default_rng(1000 + W)
    blob, off = _batch(rng)
    cols = wanted_columns(W)
    rows = _random_rows(rng, W, cols)
    want = np.zeros(W, dtype=np.uint32)
    for c in cols:
        want[c >> 5] |= np.uint32(1 << (c & 31))
    want[W - 1] |= TAIL
    for d in range(N_DOCS):
        if mode == "all":
            for c in cols:
                _set(rows, d, c, True)
        _set(rows, d, cols[d % W], bool(flags[d]) != (mode == "all"))
    return SelectCase("W = %d, %s%s" % (W, mode, "" if mode != "all" or all(flags) else ", some complete"), W, blob, off, rows, n_cols_of(W), want, mode,
                      list(flags), cols)


def route_columns(W):
    """a column in the first word, one in a middle word, and the last valid bit"""
    return [5, 32 * (W // 2) + 17 if W > 1 else 17, n_cols_of(W) - 1]


def _subset(d):
    """which of the three masks document d hits, as bits"""
    return (d * 5 + d // 8) & 7


def route_case(W, mode, rest):
    """three masks of one column each; which of them a document hits goes through all eight subsets with d"""
    rng = np.random.default_rng(2000 + W)
    blob, off = _batch(rng)
    cols = route_columns(W)
    rows = _random_rows(rng, W, cols)
    masks = np.zeros((3, W), dtype=np.uint32)
    for k, c in enumerate(cols):
        masks[k, c >> 5] |= np.uint32(1 << (c & 31))
        masks[k, W - 1] |= TAIL
        for d in range(N_DOCS):
            _set(rows, d, c, (_subset(d) >> k) & 1)
    return RouteCase("W = %d, %s%s" % (W, mode, ", rest" if rest else ""), W, blob, off, rows, n_cols_of(W), masks, mode, rest, cols)


@functools.lru_cache(maxsize=None)
def select_cases():
    rng = np.random.default_rng(7)
    out = []
    for W in WIDTHS:
        flags = (rng.random(N_DOCS) < 0.5).tolist()
        out += [select_case(W, "any", flags), select_case(W, "none", flags), select_case(W, "all", [True] * N_DOCS),
                select_case(W, "all", [d % 3 != 0 for d in range(N_DOCS)])]
    return out


@functools.lru_cache(maxsize=None)
def context_cases():
    """the select's rows under ANY, a document of context on either side"""
    return [c for c in select_cases() if c.mode == "any"]


@functools.lru_cache(maxsize=None)
def route_cases():
    return [route_case(W, mode, rest) for W in WIDTHS for mode in ("first", "every") for rest in (False, True)]


def select_ref(c, rows=None):
    return S.reference(c.blob, c.doc_off, c.rows if rows is None else rows, c.n_cols, c.want, c.mode, None)


def context_ref(c, rows=None):
    return CX.reference(c.blob, c.doc_off, c.rows if rows is None else rows, c.n_cols, c.want, c.mode, None, 1, 1, None)


def route_ref(c, rows=None):
    return R.reference(c.blob, c.doc_off, c.rows if rows is None else rows, c.n_cols, c.masks, c.mode, c.rest, None)


@functools.lru_cache(maxsize=None)
def expected():
    """{(call, name): the reference's answer}, computed once"""
    out = {("select", c.name): select_ref(c) for c in select_cases()}
    out.update({("context", c.name): context_ref(c) for c in context_cases()})
    out.update({("route", c.name): route_ref(c) for c in route_cases()})
    assert len(out) == len(select_cases()) + len(context_cases()) + len(route_cases())          # (the names are unique)
    return out


def _flipped(c, d, col):
    rows = c.rows.copy()
    rows[d, col >> 5] ^= np.uint32(1 << (col & 31))
    return rows


def assert_not_vacuous():
    """For every width and every word j, flipping the deciding bit of a document whose deciding bit lies in word j changes the
    answer of the select under every mode and of the context call; for the route, flipping a document's bit in each of the three
    mask columns does.  Lengths of 0 occur, so the document indices are compared, not the bytes alone.  The tail bits matter too."""
    n = 0
    for c in select_cases():
        ref = expected()[("select", c.name)]
        assert c.n_cols == 32 * c.W - 3 and len(c.doc_off) - 1 == N_DOCS and N_DOCS % 2 == 1
        if not (c.mode == "all" and all(c.flags)):
            assert 0 < len(ref[2]) < N_DOCS, c.name
        for j in range(c.W):
            d = j if j + c.W >= N_DOCS else j + c.W                  # (a document with d mod W == j, not the first of a wave)
            assert d % c.W == j and c.cols[j] >> 5 == j
            assert select_ref(c, _flipped(c, d, c.cols[j]))[2] != ref[2], (c.name, j)
            if c.mode == "any":
                assert context_ref(c, _flipped(c, d, c.cols[j]))[2:4] != expected()[("context", c.name)][2:4], (c.name, j)
            n += 1
        if c.mode != "all":                                          # (under ALL the rows have the tail bits the mask asks for)
            assert S.selected(c.doc_off, c.rows, c.n_cols, c.want, c.mode, None, honour_tail=True) != ref[2], c.name
    for c in route_cases():
        ref = expected()[("route", c.name)]
        assert [col >> 5 for col in c.cols] == [0, c.W // 2 if c.W > 1 else 0, c.W - 1]
        for k, col in enumerate(c.cols):
            d = next(d for d in range(8, N_DOCS) if not _subset(d) & ((1 << k) - 1))     # (no lower mask hides it under FIRST)
            assert route_ref(c, _flipped(c, d, col))[2:4] != ref[2:4], (c.name, k)
            n += 1
        assert R.reference(c.blob, c.doc_off, c.rows, c.n_cols, c.masks, c.mode, c.rest, None, honour_tail=True)[2] != ref[2], c.name
    return n
