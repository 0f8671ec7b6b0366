"""Batches for the route's tests (test_route_host.py: the kernels' walk on the host; test_gpu_route.py: the kernels): a reference
written from the contract in include/gft.h that slices Python bytes and calls neither the library nor select_docs.py's reference,
the fixed cases built from the counting tile (gft_debug_route_shape), and seeded random batches.  Every text is random bytes, so a
byte taken from the wrong place shows; the tail bits of every row's last word and of every mask are ones, so a walk that honours
them shows.  No tests in here."""
import collections
import functools

import numpy as np

from gofindthem_amd.engine import route_shape

FIRST, EVERY = 0, 1
MODES = {"first": FIRST, "every": EVERY}

Case = collections.namedtuple("Case", "name blob doc_off rows n_cols masks mode rest also")


def _int(words):
    return int.from_bytes(np.ascontiguousarray(words, dtype="<u4").tobytes(), "little")


def buckets_of(doc_off, rows, n_cols, masks, mode, rest, also, honour_tail=False):
    """[the input indices of bucket b's entries, in input order] for the B buckets, from the contract alone.  honour_tail: what a
    walk would answer that did NOT ignore the bits at and above n_cols (assert_not_vacuous)"""
    n, K = len(doc_off) - 1, len(masks)
    W = (n_cols + 31) // 32
    cut = (1 << (32 * W if honour_tail else n_cols)) - 1
    ms = [(_int(m) if W else 0) & cut for m in masks]
    mode = MODES.get(mode, mode)
    out = [[] for _ in range(K + (1 if rest else 0))]
    for d in range(n):
        if also is not None and also[d]:
            assert rest
            out[K].append(d)
            continue
        r = (_int(rows[d]) if W else 0) & cut
        hit = [k for k in range(K) if r & ms[k]]
        if mode == FIRST:
            hit = hit[:1]
        for k in hit:
            out[k].append(d)
        if rest and not hit:
            out[K].append(d)
    return out


def reference(blob, doc_off, rows, n_cols, masks, mode, rest, also, honour_tail=False):
    """(bytes, out_off, doc_idx, bucket_doc, bucket_byte) of the contract, by slicing"""
    data = bytes(blob)
    parts, off, idx, bucket_doc, bucket_byte = [], [0], [], [0], [0]
    for members in buckets_of(doc_off, rows, n_cols, masks, mode, rest, also, honour_tail):
        for d in members:
            parts.append(data[int(doc_off[d]):int(doc_off[d + 1])])
            off.append(off[-1] + len(parts[-1]))
            idx.append(d)
        bucket_doc.append(len(idx))
        bucket_byte.append(off[-1])
    return b"".join(parts), off, idx, bucket_doc, bucket_byte


def _batch(rng, lengths, lead):
    n = len(lengths)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[0] = lead
    if n:
        off[1:] = lead + np.cumsum(np.asarray(lengths, dtype=np.uint64))
    return off, rng.integers(0, 256, int(off[n]), dtype=np.uint8)


def _pack(bits, n_cols):
    """rows of booleans [r, n_cols] -> uint32 words [r, W], the tail bits of the last word ones"""
    r = bits.shape[0]
    W = (n_cols + 31) // 32
    words = np.zeros((r, max(W, 1)), dtype=np.uint32)
    for j in range(n_cols):
        words[:, j >> 5] |= bits[:, j].astype(np.uint32) << np.uint32(j & 31)
    words = words[:, :W]
    if n_cols & 31:
        words[:, W - 1] |= np.uint32((0xFFFFFFFF << (n_cols & 31)) & 0xFFFFFFFF)
    return np.ascontiguousarray(words)


def make(name, lengths, hits, K, mode="every", rest=False, also=None, n_cols=None, seed=1, lead=0):
    """a batch whose documents have `lengths` and of which document d hits exactly the buckets hits[d]: bucket k owns one column of
    its own (a seeded permutation spreads them over the words), the columns no bucket owns hold noise"""
    rng = np.random.default_rng(seed)
    n = len(lengths)
    n_cols = K + 9 if n_cols is None else n_cols
    assert n_cols >= K
    col = rng.permutation(n_cols)[:K]
    bits = rng.random((n, n_cols)) < 0.3
    bits[:, col] = False
    for d, hs in enumerate(hits):
        for k in hs:
            bits[d, col[k]] = True
    mbits = np.zeros((K, n_cols), dtype=bool)
    mbits[np.arange(K), col] = True
    off, blob = _batch(rng, lengths, lead)
    return Case(name, blob, off, _pack(bits, n_cols), n_cols, _pack(mbits, n_cols), mode, rest, None if also is None else np.asarray(also, dtype=np.uint8))


def make_width(n_cols, mode, seed):
    """three buckets over rows of n_cols columns: the last valid bit, the first bit of the last word, and column 0 with a few more"""
    rng = np.random.default_rng(seed)
    n = 150
    W = (n_cols + 31) // 32
    bits = rng.random((n, n_cols)) < 0.02
    mbits = np.zeros((3, n_cols), dtype=bool)
    if n_cols:
        mbits[0, n_cols - 1] = True
        mbits[1, 32 * (W - 1)] = True
        mbits[2, rng.integers(0, n_cols, 4)] = True
        mbits[2, 0] = True
        bits[:, n_cols - 1] = rng.random(n) < 0.3
        bits[:, 32 * (W - 1)] = rng.random(n) < 0.3
    off, blob = _batch(rng, rng.integers(0, 90, n).tolist(), 0)
    return Case("%d columns, %s" % (n_cols, mode), blob, off, _pack(bits, n_cols), n_cols, _pack(mbits, n_cols), mode, True, None)


def _random_hits(rng, n, K, p):
    return [np.flatnonzero(rng.random(K) < p).tolist() for _ in range(n)]


@functools.lru_cache(maxsize=None)
def fixed_cases():
    """every batch size, bucket count, row width and member form the contract and the tile border make special"""
    T = route_shape()
    rng = np.random.default_rng(7)
    c = []
    for n in (1, T - 1, T, T + 1, 2 * T + 1):
        c.append(make("%d documents" % n, rng.integers(0, 70, n).tolist(), _random_hits(rng, n, 3, 0.4), 3, rest=True, seed=10 + n, lead=5 if n == T else 0))
    # empty documents at bucket 0's start and end, as the whole of bucket 1; bucket 2 starts with bytes
    c.append(make("empty documents at a bucket's borders and as a whole bucket", [0, 7, 0, 0, 0, 9, 4], [[0], [0], [0], [1], [1], [2], []], 3, seed=20))
    c.append(make("only the last document is routed", [30] * (2 * T + 1), [[]] * (2 * T) + [[1]], 2, seed=21, lead=5))
    c.append(make("doc_off[0] = 5", [11, 0, 40, 3], [[1], [0], [0, 1], []], 2, rest=True, seed=22, lead=5))
    for K, rest in ((1, False), (2, False), (63, False), (64, False), (63, True), (0, True), (1, True)):
        n = T + 9
        c.append(make("%d masks%s" % (K, ", rest" if rest else ""), rng.integers(0, 50, n).tolist(), _random_hits(rng, n, K, 2.0 / max(K, 1)), K, rest=rest,
                      seed=30 + K + rest))
    n = T + 5
    c.append(make("buckets 0, 2 and 4 stay empty", rng.integers(0, 50, n).tolist(), [[1] if d % 3 == 0 else [3] if d % 3 == 1 else [1, 3] for d in range(n)], 5,
                  seed=40))
    c.append(make("every document in the last bucket", rng.integers(0, 50, n).tolist(), [[63]] * n, 64, seed=41))
    c.append(make("a document in all 64 buckets", rng.integers(1, 50, n).tolist(), [list(range(64)) if d == T - 1 else [d % 64] for d in range(n)], 64, seed=42))
    for mode in ("first", "every"):
        c.append(make("a document hits buckets 3 and 7, %s" % mode, [5, 6, 7, 8], [[7], [3, 7], [3], [0, 3, 7]], 9, mode=mode, seed=43))
    c.append(make("no rest and no hit", [5, 6, 7], [[], [], []], 4, seed=44))
    c.append(make("no rest, one document absent", [5, 6, 7], [[0], [], [1]], 2, seed=45))
    c.append(make("no masks, no rest", [5, 6, 7], [[], [], []], 0, seed=46))
    c.append(make("no masks, rest", [5, 0, 7], [[], [], []], 0, rest=True, seed=47, lead=3))
    for n_cols in (0, 31, 32, 33, 40, 65, 2048, 2080):
        for mode in ("first", "every"):
            c.append(make_width(n_cols, mode, 100 + n_cols))
    n = 80
    also = np.zeros(n, dtype=np.uint8)
    also[[0, 5, 6, 40, 79]] = [1, 2, 255, 7, 1]
    hits = _random_hits(rng, n, 6, 0.3)
    hits[0], hits[5], hits[40] = [0, 2], [1], [0, 1, 2, 3, 4, 5]          # documents whose rows hit masks
    for mode in ("first", "every"):
        c.append(make("also, %s" % mode, rng.integers(0, 120, n).tolist(), hits, 6, mode=mode, rest=True, also=also, seed=50))
    c.append(make("also all zero", rng.integers(0, 120, n).tolist(), hits, 6, rest=True, also=np.zeros(n, dtype=np.uint8), seed=51))
    # the scans' tile of 4 096 entries: 64 buckets x 65 tiles of documents -- the count table crosses a scan block, the bucket bases
    # come from the spine -- and more than 4 096 entries for the offset scan
    n = 65 * T
    c.append(make("64 buckets, 65 tiles", rng.integers(0, 12, n).tolist(), _random_hits(rng, n, 64, 2.0 / 64), 64, seed=60, lead=1))
    c.append(make("5000 entries in two buckets", rng.integers(0, 9, 2600).tolist(), [[0, 1]] * 2500 + [[]] * 100, 2, rest=True, seed=61))
    return c


@functools.lru_cache(maxsize=None)
def random_cases(count=200):
    """seeded small batches: every bucket count, width, density, mode and flag at random"""
    rng = np.random.default_rng(20240913)
    out = []
    for i in range(count):
        n = int(rng.integers(0, 200))
        K = int(rng.choice([0, 1, 2, 3, 5, 8, 17, 32, 63, 64]))
        rest = bool(rng.integers(0, 2)) and K < 64
        n_cols = int(rng.choice([0, 1, 7, 31, 32, 33, 40, 64, 65, 100, 257]))
        mode = ("first", "every")[int(rng.integers(0, 2))]
        bits = rng.random((n, n_cols)) < rng.choice([0.005, 0.05, 0.5])
        mbits = rng.random((K, n_cols)) < rng.choice([0.02, 0.2])
        also = (rng.random(n) < 0.05).astype(np.uint8) if rest and i % 3 == 0 else None
        short = rng.integers(0, 40, n)
        lens = np.where(rng.random(n) < 0.9, short, rng.integers(0, 5000, n))
        off, blob = _batch(rng, lens.tolist(), i % 7)
        out.append(Case("random %d: %d documents, %d masks, %d columns, %s%s" % (i, n, K, n_cols, mode, ", rest" if rest else ""), blob, off,
                        _pack(bits, n_cols), n_cols, _pack(mbits, n_cols), mode, rest, also))
    return out


def all_cases():
    return fixed_cases() + random_cases()


@functools.lru_cache(maxsize=None)
def expected():
    """{name: (bytes, out_off, doc_idx, bucket_doc, bucket_byte)} of all_cases(), computed once"""
    return {c.name: reference(c.blob, c.doc_off, c.rows, c.n_cols, c.masks, c.mode, c.rest, c.also) for c in all_cases()}


def case(name):
    return next(c for c in fixed_cases() if c.name == name)


def assert_not_vacuous():
    """the tail bits matter: a walk that honoured the bits at and above n_cols would answer some fixed case differently; and the
    fixed cases route neither nothing nor everything throughout"""
    flips = [c.name for c in fixed_cases() if c.n_cols & 31 and
             reference(c.blob, c.doc_off, c.rows, c.n_cols, c.masks, c.mode, c.rest, c.also, honour_tail=True)[2] != expected()[c.name][2]]
    assert flips, "no case would notice a walk that honours the tail bits"
    names = set(c.name for c in all_cases())
    assert len(names) == len(all_cases())
    some = [c.name for c in fixed_cases() if 0 < len(expected()[c.name][2]) and len(set(expected()[c.name][2])) < len(c.doc_off) - 1]
    twice = [c.name for c in fixed_cases() if len(expected()[c.name][2]) > len(set(expected()[c.name][2]))]
    assert len(some) > 5 and len(twice) > 5
    return flips
