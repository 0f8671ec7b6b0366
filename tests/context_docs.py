"""Batches for the context call's tests (test_context_host.py: the kernels' walk on the host; test_gpu_context.py: the kernels): a
reference written from the contract in include/gft.h -- a brute force over the selected documents that slices and does not call
the library --, a handful of deliberately wrong references, the fixed cases built from the kernels' own borders
(gft_debug_context_shape), and seeded random batches.  The batches themselves are made by select_docs.make: random bytes, tail bits
of rows and masks all ones.  No tests in here."""
import collections
import functools

import numpy as np

import select_docs as S
from gofindthem_amd.engine import context_shape

U64 = (1 << 64) - 1
REACHES = (0, 1, 2, 5, 63, 64, 65, 700, U64)

Case = collections.namedtuple("Case", "name blob doc_off rows n_cols want mode also before after fence")

# the wrong references: what a walk with one plausible mistake would answer
WRONG = ("swapped", "after short", "after long", "before short", "before long", "no fences", "fence late", "groups unsplit", "tile stop",
         "carry stop", "wrap", "also draws nothing")


def keep_flags(n, sel, before, after, fence, stop=0, wrap=False):
    """which of n documents are kept: for every selected h the documents d with d - after <= h <= d + before and no fence index
    in (min(h, d), max(h, d)].  stop: a reach that does not leave h's run of `stop` documents; wrap: d + before taken modulo 2^64"""
    keep = np.zeros(n, dtype=bool)
    fpos = np.flatnonzero(fence) if fence is not None else np.zeros(0, dtype=np.int64)
    for h in sel:
        h = int(h)
        hi = min(n - 1, h + after)                       # behind h: d in (h, h + after], no fence in (h, d]
        nxt = fpos[fpos > h]
        if nxt.size:
            hi = min(hi, int(nxt[0]) - 1)
        lo = max(0, h - before)                          # in front of h: d in [h - before, h), no fence in (d, h]
        prv = fpos[fpos <= h]
        if prv.size:
            lo = max(lo, int(prv[-1]))
        if stop:
            lo, hi = max(lo, h // stop * stop), min(hi, h // stop * stop + stop - 1)
        front_hi = min(h - 1, U64 - before) if wrap else h - 1
        if lo <= front_hi:
            keep[lo:front_hi + 1] = True
        keep[h:hi + 1] = True
    return keep


def reference(blob, doc_off, rows, n_cols, want, mode, also, before, after, fence, wrong=None):
    """(bytes, out_off, doc_idx, kind, group_off) of the contract, by slicing; wrong: one of WRONG"""
    data = bytes(blob)
    n = len(doc_off) - 1
    before, after = int(before), int(after)
    fence = None if fence is None else np.asarray(fence) != 0
    sel = S.selected(doc_off, rows, n_cols, want, mode, also)
    draws, group_fence, stop = sel, fence, 0
    if wrong == "swapped":
        before, after = after, before
    elif wrong == "after short":
        after = max(after - 1, 0)
    elif wrong == "after long":
        after = min(after + 1, U64)
    elif wrong == "before short":
        before = max(before - 1, 0)
    elif wrong == "before long":
        before = min(before + 1, U64)
    elif wrong == "no fences":
        fence = group_fence = None
    elif wrong == "fence late" and fence is not None:
        fence = group_fence = np.concatenate([[False], fence[:-1]])
    elif wrong == "groups unsplit":
        group_fence = None
    elif wrong == "tile stop":
        stop = context_shape()[0]
    elif wrong == "carry stop":
        stop = context_shape()[0] * context_shape()[1]
    elif wrong == "also draws nothing":
        draws = S.selected(doc_off, rows, n_cols, want, mode, None)
    keep = keep_flags(n, draws, before, after, fence, stop, wrong == "wrap")
    keep[sel] = True
    idx = np.flatnonzero(keep).tolist()
    hit = set(sel)
    parts = [data[int(doc_off[d]):int(doc_off[d + 1])] for d in idx]
    off = [0]
    for p in parts:
        off.append(off[-1] + len(p))
    groups = [r for r, d in enumerate(idx) if r == 0 or idx[r - 1] != d - 1 or (group_fence is not None and group_fence[d])]
    return b"".join(parts), off, idx, [1 if d in hit else 0 for d in idx], groups + [len(idx)]


def make(name, n, hits, before, after, fences=(), seed=1, lengths=None, **kw):
    """n documents of 0 to 40 bytes, those at `hits` selected (a list of indices, or flags), fences at `fences`; kw: select_docs.make's"""
    rng = np.random.default_rng(seed)
    flags = np.zeros(n, dtype=bool)
    hits = np.asarray(hits)
    if hits.dtype == bool:
        flags[:] = hits
    elif hits.size:
        flags[hits.astype(np.int64)] = True
    if lengths is None:
        lengths = rng.integers(0, 41, n).tolist()
    c = S.make(name, lengths, flags.tolist(), seed=seed, **kw)
    fence = None
    if fences is not None:
        fence = np.zeros(n, dtype=np.uint8)
        f = np.asarray(fences)
        if f.dtype == bool:
            fence[f] = 1
        elif f.size:
            fence[f.astype(np.int64)] = rng.integers(1, 256, f.size)            # (any non-zero byte is a fence)
    return Case(c.name, c.blob, c.doc_off, c.rows, c.n_cols, c.want, c.mode, c.also, before, after, fence)


@functools.lru_cache(maxsize=None)
def fixed_cases():
    """the smallest shapes at which a tile, a carry block, a reach or a fence can go wrong"""
    T, CB, SPINE = context_shape()
    B = T * CB                                            # documents per carry block
    rng = np.random.default_rng(4242)
    c = []
    for n in (1, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1):
        flags = rng.random(n) < 0.08
        flags[rng.integers(0, n)] = True
        c.append(make("%d documents" % n, n, flags, 1, 2, seed=10 + n))
        c.append(make("%d documents, fences" % n, n, flags, 3, 1, fences=rng.random(n) < 0.1, seed=20 + n, lead=3))
        c.append(make("%d documents, the last one hit" % n, n, [n - 1], 2, 2, seed=30 + n))
    # the carry-block border, one tile either side of it
    n = B + T + 5
    c += [make("a hit in front of the carry border, context behind it", n, [B - 1], 0, 3, seed=40),
          make("a hit behind the carry border, context in front of it", n, [B], 3, 0, seed=41),
          make("hits in the tiles either side of the carry border", n, [B - T + 3, B + T - 3], T - 5, T - 5, seed=42),
          make("a hit a tile in front of the carry border reaches over it", n, [B - T - 1], 0, T + 2, seed=43),
          make("a hit a tile behind the carry border reaches over it", n, [B + T], T + 1, 0, seed=44),
          make("a fence at the carry border", n, [B - 2, B + 1], 5, 5, fences=[B], seed=45),
          make("a fence behind the carry border", n, [B - 2], 5, 5, fences=[B + 1], seed=46)]
    # a lone hit
    n = 3 * T + 8
    c += [make("a lone hit at 0", n, [0], 3, 3, seed=50),
          make("a lone hit at n - 1", n, [n - 1], 3, 3, seed=51),
          make("a lone hit in the last lane, after 1", n, [2 * T - 1], 0, 1, seed=52),
          make("a lone hit in the first lane, before 1", n, [2 * T], 1, 0, seed=53),
          make("a lone hit in the last lane, before 1", n, [2 * T - 1], 1, 0, seed=54),
          make("a lone hit in the first lane, after 1", n, [2 * T], 0, 1, seed=55)]
    # long reaches over k empty tiles
    for k in (1, 3):
        n = (k + 2) * T + 9
        for r in (T * k - 1, T * k, T * k + 1):
            c.append(make("after %d over %d empty tiles" % (r, k), n, [10], 0, r, seed=60 + k))
            c.append(make("before %d over %d empty tiles" % (r, k), n, [n - 11], r, 0, seed=62 + k))
            c.append(make("both %d over %d empty tiles, lane 63" % (r, k), n, [T - 1, n - 1], r, r, seed=64 + k))
    n = 2 * B + 100
    c += [make("a reach longer than a carry block, behind", n, [5], 0, B + 70, seed=70),
          make("a reach longer than a carry block, in front", n, [n - 3], B + 70, 0, seed=71),
          make("a reach longer than a carry block, a fence in its way", n, [5, n - 3], B + 70, B + 70, fences=[B + 9, B + 11], seed=72)]
    # more carry blocks than one trip of the spine resolves: the carries travel from trip to trip, forward and backward
    n = (SPINE + 1) * B + 2 * T
    short = np.random.default_rng(73).integers(0, 4, n).tolist()
    c += [make("a reach over more carry blocks than a trip of the spine, behind", n, [5], 0, U64, fences=[n - 7], seed=73, lengths=short, n_cols=3),
          make("a reach over more carry blocks than a trip of the spine, in front", n, [n - 3], U64, 0, fences=[9], seed=74, lengths=short, n_cols=3)]
    n = 300
    c += [make("before 2^64 - 1", n, [150], U64, 0, fences=[40, 260], seed=80),
          make("after 2^64 - 1", n, [150], 0, U64, fences=[40, 260], seed=81),
          make("both 2^64 - 1, no fence", n, [150], U64, U64, fences=None, seed=82),
          make("both 2^64 - 1, hits at either end", n, [0, n - 1], U64, U64, fences=[100, 200], seed=83),
          make("before 2^64 - 2", n, [150], U64 - 1, 1, seed=84)]
    # nothing, everything
    c += [make("nothing selected", 130, [], 2, 2, fences=[5, 64], seed=90),
          make("everything selected", 130, np.ones(130, dtype=bool), 2, 2, seed=91),
          make("everything selected, a fence on every document", 130, np.ones(130, dtype=bool), 2, 2, fences=np.ones(130, dtype=bool), seed=92),
          make("every other one selected, no reach", 130, np.arange(0, 130, 2), 0, 0, seed=93)]
    # two hits whose contexts touch, overlap, or leave a gap of exactly one document -- inside a tile and over a tile border
    for a in (20, T - 3):
        for gap, what in ((3, "touch"), (2, "overlap"), (4, "leave one out")):
            c.append(make("two hits at %d whose contexts %s" % (a, what), 2 * T + 3, [a, a + gap], 1, 1, seed=100 + a + gap))
    # fences
    n = 2 * T + 20
    c += [make("a fence at 0", n, [0, 3], 5, 5, fences=[0], seed=110),
          make("a fence at 0 alone, a hit at 1", n, [1], 5, 5, fences=[0], seed=111),
          make("a fence at the tile border, hits either side", n, [T - 2, T + 2], 5, 5, fences=[T], seed=112),
          make("a fence in the last lane, hits either side", n, [T - 3, T + 1], 5, 5, fences=[T - 1], seed=113),
          make("a fence right behind a hit", n, [30], 3, 3, fences=[31], seed=114),
          make("a fence on the hit itself", n, [30], 3, 3, fences=[30], seed=115),
          make("a fence on a hit whose neighbour is hit too", n, [29, 30, 31], 1, 1, fences=[30], seed=116),
          make("a fence inside a run of context", n, [30, 36], 3, 3, fences=[33], seed=117),
          make("a fence on every document", n, [7, T, T + 1, n - 1], 4, 4, fences=np.ones(n, dtype=bool), seed=118),
          make("a fence on every document but one", n, [7, T], 4, 4, fences=np.arange(n) != T, seed=119)]
    # the row widths: the three routes of k_select_mark, and no rows at all
    n = 150
    flags = rng.random(n) < 0.06
    for n_cols in (0, 20, 70, 65 * 32):
        for mode in ("any", "all", "none"):
            also = np.zeros(n, dtype=np.uint8)
            also[[3, 77, 140]] = [1, 200, 5]
            c.append(make("%d columns, %s, also" % (n_cols, mode), n, flags, 2, 1, fences=[70, 78], n_cols=n_cols, mode=mode, also=also,
                          want=None if n_cols == 0 else "some", seed=120 + n_cols % 97))
            c.append(make("%d columns, %s" % (n_cols, mode), n, flags, 1, 2, n_cols=n_cols, mode=mode, want=None if n_cols == 0 else "some",
                          seed=130 + n_cols % 97))
    also = np.zeros(n, dtype=np.uint8)
    also[[10, 100]] = 1
    c.append(make("also alone draws context", n, [], 2, 2, n_cols=33, also=also, seed=140))
    # empty documents as hits and as context; text that does not begin at 0
    lens = [0] * 12 + [7] + [0] * 12
    c += [make("empty documents round a hit", 25, [12], 3, 3, lengths=lens, seed=150),
          make("an empty hit among empty context", 25, [5], 2, 2, lengths=lens, seed=151),
          make("only empty documents", 70, [3, 66], 1, 1, lengths=[0] * 70, seed=152),
          make("text that begins at 7", 100, [0, 50, 99], 2, 2, fences=[51], seed=153, lead=7)]
    return c


@functools.lru_cache(maxsize=None)
def random_cases():
    """200 seeded batches of up to 700 documents; before and after from REACHES"""
    rng = np.random.default_rng(20250909)
    out = []
    for i in range(200):
        n = int(rng.integers(1, 701))
        density = (0.005, 0.05, 0.3)[i % 3]
        fd = (None, 0.02, 0.3)[(i // 3) % 3]
        before, after = (REACHES[int(k)] for k in rng.integers(0, len(REACHES), 2))
        n_cols, mode = (5, 33, 70)[i % 3], ("any", "all", "none")[(i // 2) % 3]
        also = (rng.random(n) < 0.01).astype(np.uint8) if i % 5 == 4 else None
        out.append(make("random %d: %d documents, %g, fences %s, before %d, after %d, %s" % (i, n, density, fd, before, after, mode), n,
                        rng.random(n) < density, before, after, fences=None if fd is None else rng.random(n) < fd, n_cols=n_cols, mode=mode,
                        also=also, seed=5000 + i, lead=i % 4))
    return out


def all_cases():
    return fixed_cases() + random_cases()


def ref_of(c, wrong=None):
    return reference(c.blob, c.doc_off, c.rows, c.n_cols, c.want, c.mode, c.also, c.before, c.after, c.fence, wrong)


@functools.lru_cache(maxsize=None)
def expected():
    """{name: (bytes, out_off, doc_idx, kind, group_off)} of all_cases(), computed once"""
    out = {c.name: ref_of(c) for c in all_cases()}
    assert len(out) == len(all_cases()), "two cases of one name"
    return out


def assert_not_vacuous():
    """every wrong reference is told from the right one by some case, and by a fixed one; the cases keep neither nothing nor
    everything throughout, and some have context, several groups and fences that split a run"""
    want = expected()
    told = {}
    T, CB, SPINE = context_shape()
    short = [c for c in fixed_cases() if len(c.doc_off) < 4 * T * CB]   # (the two cases of the spine's trips are long and tell nothing here)
    for w in WRONG:
        told[w] = [c.name for c in short if ref_of(c, w) != want[c.name]]
        assert told[w], "no fixed case would notice the wrong reference %r" % w
        if w != "carry stop":                                # (no random batch is as long as a carry block)
            assert any(ref_of(c, w) != want[c.name] for c in random_cases()), "no random case would notice the wrong reference %r" % w
    some = [c.name for c in all_cases() if 0 < len(want[c.name][2]) < len(c.doc_off) - 1]
    assert len(some) > 100
    assert sum(1 for v in want.values() if 0 in v[3] and 1 in v[3]) > 100 and sum(1 for v in want.values() if len(v[4]) > 3) > 50
    return told
