"""Batches for the select's tests (test_select_host.py: the kernels' walk on the host; test_gpu_select.py: the kernels): a reference
written from the contract in include/gft.h that slices and does not call the library, the fixed cases built from the copy kernel's
own borders (gft_debug_select_shape), and seeded random batches.  Every text is random bytes, so a byte taken from the wrong place
shows; the tail bits of every row's last word and of every mask are ones, so a walk that honours them shows.  No tests in here."""
import collections
import functools

import numpy as np

from gofindthem_amd.engine import select_shape

ANY, ALL, NONE = 0, 1, 2
MODES = {"any": ANY, "all": ALL, "none": NONE}

Case = collections.namedtuple("Case", "name blob doc_off rows n_cols want mode also")


def _ints(words):
    return int.from_bytes(np.ascontiguousarray(words, dtype="<u4").tobytes(), "little")


def selected(doc_off, rows, n_cols, want, mode, also, honour_tail=False):
    """the input indices of the selected documents, from the contract alone.  honour_tail: what a walk would answer that did NOT
    ignore the bits at and above n_cols (assert_not_vacuous)"""
    n = len(doc_off) - 1
    W = (n_cols + 31) // 32
    mask = (1 << (32 * W if honour_tail else n_cols)) - 1
    w = (mask if want is None else _ints(want)) & mask
    mode = MODES.get(mode, mode)
    out = []
    for d in range(n):
        r = (_ints(rows[d]) if W else 0) & w
        hit = r != 0 if mode == ANY else r == w if mode == ALL else r == 0
        if hit or (also is not None and also[d]):
            out.append(d)
    return out


def reference(blob, doc_off, rows, n_cols, want, mode, also, honour_tail=False):
    """(bytes, out_off, doc_idx) of the contract, by slicing"""
    data = bytes(blob)
    idx = selected(doc_off, rows, n_cols, want, mode, also, honour_tail)
    parts = [data[int(doc_off[d]):int(doc_off[d + 1])] for d in idx]
    off = [0]
    for p in parts:
        off.append(off[-1] + len(p))
    return b"".join(parts), off, idx


def make(name, lengths, flags, n_cols=40, mode="any", want="some", also=None, seed=1, lead=0):
    """a batch whose documents have `lengths` and of which those with a true flag are selected under `mode`: rows and mask are
    drawn so.  want: "some" (a random non-empty set of columns), None, "empty" (flags are then ignored: the contract decides).
    lead: junk bytes in front of document 0 (doc_off[0] = lead)"""
    rng = np.random.default_rng(seed)
    n = len(lengths)
    W = (n_cols + 31) // 32
    off = np.zeros(n + 1, dtype=np.uint64)
    off[0] = lead
    if n:
        off[1:] = lead + np.cumsum(np.asarray(lengths, dtype=np.uint64))
    blob = rng.integers(0, 256, int(off[n]), dtype=np.uint8)
    flags = np.asarray(flags, dtype=bool)
    cols = np.zeros(n_cols, dtype=bool)
    if want == "some" and n_cols:
        cols[rng.integers(0, n_cols, max(1, n_cols // 7))] = True
    elif want is None:
        cols[:] = True
    bits = rng.random((n, n_cols)) < 0.3
    m = MODES[mode]
    if cols.any():
        first = np.flatnonzero(cols)
        pick = first[rng.integers(0, len(first), n)]                    # one wanted column per document
        if m in (ANY, NONE):
            hit = flags if m == ANY else ~flags
            bits[:, cols] &= hit[:, None]
            bits[np.flatnonzero(hit), pick[hit]] = True
        else:
            bits[:, cols] |= flags[:, None]
            bits[np.flatnonzero(~flags), pick[~flags]] = False
    rows = np.zeros((n, max(W, 1)), dtype=np.uint32)
    for j in range(n_cols):
        rows[:, j >> 5] |= bits[:, j].astype(np.uint32) << np.uint32(j & 31)
    rows = rows[:, :W]
    wm = None
    if want is not None:
        wm = np.zeros(max(W, 1), dtype=np.uint32)
        for j in np.flatnonzero(cols):
            wm[j >> 5] |= np.uint32(1 << (j & 31))
        wm = wm[:W]
    if n_cols & 31:                                                     # the tail bits: ones everywhere
        tail = np.uint32((0xFFFFFFFF << (n_cols & 31)) & 0xFFFFFFFF)
        rows[:, W - 1] |= tail
        if wm is not None:
            wm[W - 1] |= tail
    al = None if also is None else np.asarray(also, dtype=np.uint8)
    return Case(name, blob, off, np.ascontiguousarray(rows), n_cols, wm, mode, al)


def _alternate(n, first=True):
    return [(i % 2 == 0) == first for i in range(n)]


@functools.lru_cache(maxsize=None)
def fixed_cases():
    """every length, run and mask form the contract and the chunk / trip / tile borders make special"""
    C, TRIP, TILE = select_shape()
    edge = [0, 1, C - 1, C, C + 1, TRIP - 1, TRIP, TRIP + 1, TILE - 1, TILE + 1, 3 * TILE + 5]
    c = [make("edge lengths, all selected", edge, [True] * len(edge), seed=2),
         make("edge lengths, every other one", edge + edge, _alternate(2 * len(edge)), seed=3, lead=7),
         make("edge lengths, the other ones", edge + edge, _alternate(2 * len(edge), False), seed=4),
         make("40 empty documents between two bytes", [5, 1] + [0] * 40 + [1, 9], [False] + [True] * 42 + [False], seed=5),
         make("40 empty documents in front", [0] * 40 + [1, 9], [True] * 42, seed=6),
         make("40 empty documents at the end", [3] + [0] * 40, [True] * 41, seed=7),
         make("300 empty documents between two chunks", [9, C] + [0] * 300 + [C, 9], [False] + [True] * 302 + [False], seed=21),
         make("300 empty documents at the start of a trip", [TRIP] + [0] * 300 + [1, 40], [True] * 303, seed=22),
         make("500 empty documents in front, some of them", [0] * 500 + [TILE + 3], [i % 3 != 1 for i in range(500)] + [True], seed=23),
         make("200 one-byte documents", [1] * 200, [True] * 200, seed=8),
         make("2000 one-byte documents, a third of them", [1] * 2000, [i % 3 == 0 for i in range(2000)], seed=9, lead=3),
         make("200 documents of 0 to 3 bytes", [i % 4 for i in range(200)], [True] * 200, seed=10),
         make("a long unselected stretch", [100] * 3 + [2 * TILE + 7] * 5 + [50] * 300 + [100] * 3, [True] * 3 + [False] * 305 + [True] * 3, seed=11),
         make("only empty documents selected", [0, 8, 0, 8, 0], [True, False, True, False, True], seed=12),
         make("nothing selected", [30] * 50, [False] * 50, seed=13),
         make("everything selected", [30] * 50 + [TILE + 3], [True] * 51, seed=14),
         make("one document", [TRIP + 5], [True], seed=15),
         make("one document, not selected", [TRIP + 5], [False], seed=16)]
    for a in (True, False):
        for b in (True, False):
            c.append(make("first %s, last %s" % (a, b), [37, 64, 5, 90], [a, False, True, b], seed=17 + 2 * a + b, lead=2 * a))
    rng = np.random.default_rng(99)
    for n_cols in (1, 31, 32, 33, 70, 2048, 2081):
        for mode in ("any", "all", "none"):
            n = 150
            c.append(make("%d columns, %s" % (n_cols, mode), rng.integers(0, 300, n).tolist(), (rng.random(n) < 0.4).tolist(), n_cols=n_cols,
                          mode=mode, seed=100 + n_cols))
    for mode in ("any", "all", "none"):
        n = 60
        lens = rng.integers(0, 200, n).tolist()
        c += [make("every column, %s" % mode, lens, (rng.random(n) < 0.5).tolist(), n_cols=45, mode=mode, want=None, seed=200),
              make("empty mask, %s" % mode, lens, [False] * n, n_cols=45, mode=mode, want="empty", seed=201),
              make("no columns, %s" % mode, lens, [False] * n, n_cols=0, mode=mode, want=None, seed=202),
              make("no columns, a mask of no words, %s" % mode, lens, [False] * n, n_cols=0, mode=mode, want="empty", seed=203)]
    n = 80
    also = np.zeros(n, dtype=np.uint8)
    also[[0, 5, 6, 40, 79]] = [1, 2, 255, 7, 1]
    flags = rng.random(n) < 0.2
    flags[[0, 5, 40]] = False                                           # documents whose row says no
    for mode in ("any", "all", "none"):
        c.append(make("also, %s" % mode, rng.integers(0, 120, n).tolist(), flags.tolist(), n_cols=33, mode=mode, also=also, seed=300))
    c.append(make("also alone", [20] * n, [False] * n, n_cols=0, also=also, seed=301))
    return c


@functools.lru_cache(maxsize=None)
def random_cases():
    """seeded batches of up to 5 000 documents, rows at densities 0.5 %, 10 % and 90 %"""
    rng = np.random.default_rng(20240707)
    out = []
    for i, (n, density, n_cols, mode) in enumerate([(5000, 0.005, 40, "any"), (5000, 0.1, 70, "any"), (5000, 0.9, 33, "any"), (3000, 0.005, 2081, "all"),
                                                    (3000, 0.1, 31, "none"), (3000, 0.9, 64, "all"), (700, 0.005, 5, "none"), (700, 0.1, 2048, "any"),
                                                    (700, 0.9, 100, "none")]):
        short = rng.integers(0, 40, n)
        lens = np.where(rng.random(n) < 0.8, short, rng.integers(0, 3000, n))
        also = (rng.random(n) < 0.01).astype(np.uint8) if i % 3 == 2 else None
        out.append(make("random %d: %d documents, %g, %d columns, %s" % (i, n, density, n_cols, mode), lens.tolist(), (rng.random(n) < density).tolist(),
                        n_cols=n_cols, mode=mode, also=also, seed=1000 + i, lead=i))
    return out


def all_cases():
    return fixed_cases() + random_cases()


@functools.lru_cache(maxsize=None)
def expected():
    """{name: (bytes, out_off, doc_idx)} of all_cases(), computed once"""
    return {c.name: reference(c.blob, c.doc_off, c.rows, c.n_cols, c.want, c.mode, c.also) for c in all_cases()}


def assert_not_vacuous():
    """the tail bits matter: some case's answer would flip if the bits at and above n_cols were honoured, and the cases select
    neither nothing nor everything throughout"""
    flips = [c.name for c in all_cases() if c.n_cols & 31 and
             selected(c.doc_off, c.rows, c.n_cols, c.want, c.mode, c.also, honour_tail=True) != expected()[c.name][2]]
    assert flips, "no case would notice a walk that honours the tail bits"
    some = [c.name for c in all_cases() if 0 < len(expected()[c.name][2]) < len(c.doc_off) - 1]
    assert len(some) > 20
    return flips
