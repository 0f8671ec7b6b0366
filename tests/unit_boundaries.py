"""Batches for the boundary between two work units of k_scan5 (test infrastructure: numpy only, no GPU, no tests in here).  At
the top of a unit every lane loads four bytes of history and its first 16-byte piece; whether that happens there or -- as the
experiments of DESIGN.md 4.1c tried -- ahead of time under the flush of the unit before, with clamped addresses, these are the
places where it can go wrong: every kind of unit behind every kind of unit, and text that must not be matched on every side such
a load can reach.  Run on one CU (schema_scale.ONE_CU) the 16 waves of one workgroup take all units in turn, so every wave has a
next unit several times and the last ones have none.

    pairs        documents of 0 .. 257 bytes: every (length class, length class) at unit distances 1 and 16
    empty_run    20 empty documents, then a document at blob offset 0 with keywords in its first bytes: a wave's NEXT unit
                 within four bytes of the blob's start; with 1, 3 and 4 lead bytes that would complete a cut keyword
    blob_end     the last document ends on the blob's last byte with a keyword; the slack completes longer ones
    long_doc     a 40 000-byte document between short ones (the next unit lies in the same document), keywords across every
                 unit border at 8 192- and 512-byte units; dense enough that a second call runs at 512-byte units
    second_walk  units whose matches outgrow the wave's fifo (walked a second time in front of the flush) among ordinary ones

Dictionary and expressions are placement.py's; expectations come from oracle.pyoracle on the bare documents."""
import collections
import functools

import numpy as np

import placement as pl
from oracle.pyoracle import POS_START, Oracle, pack_strings
from presence_once import unit_bytes

TERMS = pl.TERMS_ASCII
LENGTHS = (0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257)
# what the first bytes of a unit look like to the wave: no byte; fewer than a lane's four; a few lanes; 16 lanes; all 64 (a
# lane owns four bytes of a unit of up to 256, so in the first four classes lanes have nothing: nvalid == 0)
CLASSES = ((0,), (1, 2, 3), (4, 5, 15, 16, 17), (63, 64, 65), (255, 256, 257))
WAVES = 16                          # of the one workgroup: at an even pace a wave's next unit is 16 further
LEADS = (0, 1, 3, 4)
LEAD = b"kzxq"                      # its last 1, 3 or 4 bytes in front of "7.7": "q7" lies across doc_off[0], "zxq" in front of it
LONG_DOC = 40_000
UNIT_SIZES = (8192, 512)

Case = collections.namedtuple("Case", "name docs lead tail")


def class_of(n):
    return next(k for k, c in enumerate(CLASSES) if n in c)


def _rng(*salt):
    return np.random.default_rng([20261020, *salt])


def _text(rng, n):
    """n bytes that hold keywords: dense text of the dictionary, cut to length (tiny documents start with short keywords)"""
    if n <= 5:
        return (b"q7.7 ", b"zxq7 ", b"kjq7.", b"7.7q ", b"wxyz ")[int(rng.integers(5))][:n]
    return pl._dense(rng, TERMS, n + 40)[:n]


def _circuit():
    """every ordered pair of the five classes as consecutive entries: an Eulerian circuit of the complete digraph with loops"""
    k = len(CLASSES)
    left = {a: list(range(k)) for a in range(k)}
    stack, out = [0], []
    while stack:
        a = stack[-1]
        if left[a]:
            stack.append(left[a].pop())
        else:
            out.append(stack.pop())
    out.reverse()
    assert len(out) == k * k + 1 and out[0] == out[-1]
    return out


def _pairs():
    rng = _rng(1)
    e = _circuit()[:-1]                                  # 25 classes, read cyclically
    blocks = len(e) - WAVES + 2                          # unit i has class e[i // 16 + i % 16]: shifts 0 .. 25 at both distances
    docs, turn = [], collections.Counter()
    for i in range(blocks * WAVES):
        c = e[(i // WAVES + i % WAVES) % len(e)]
        n = CLASSES[c][turn[c] % len(CLASSES[c])]
        turn[c] += 1
        docs.append(_text(rng, n))
    return Case("pairs", docs, b"", b"")


def pair_coverage(docs, distance):
    """the (class, class) pairs of documents `distance` apart"""
    cls = [class_of(len(d)) for d in docs]
    return {(cls[i], cls[i + distance]) for i in range(len(cls) - distance)}


def _ordinary(rng, n):
    return [_text(rng, int(m)) for m in rng.integers(20, 400, n)]


def _empty_run(lead_len):
    rng = _rng(2)
    first = b"7.7 q7 " + pl.T10 + b" " + _text(rng, 300)   # "7" at offset 0, "7.7" at 0..2: the start rule of the short terms
    docs = [b""] * 20 + [first] + _ordinary(rng, 30)
    return Case("empty_run_lead%d" % lead_len, docs, LEAD[len(LEAD) - lead_len:], b"")


def _blob_end():
    rng = _rng(3)
    last = _text(rng, 150) + b" " + pl.E10[:6]           # "nation" (and "tion") end on the blob's last byte
    tail = pl.E10[6:] + pl.E33[len(pl.E10):]             # ... and the slack goes on: "nationwide", E33, "nations" must not match
    return Case("blob_end", _ordinary(rng, 44) + [b"", last], b"", tail)


def unit_borders(n, unit_max):
    per = unit_bytes(n, unit_max)
    return list(range(per, n, per))


def _long_doc():
    """"nationals" back to back: four entries per nine bytes, all of keywords of four bytes and more, so that a presence-only
    scan learns the same density as one with positions; keywords of every length class across the borders of both unit sizes"""
    rng = _rng(4)
    body = bytearray((b"nationals" * (LONG_DOC // 9 + 1))[:LONG_DOC])
    across = [pl.T10, b"q7", pl.T24, b"kjq", pl.T33, b"wxyz", pl.T26, b"zxq", pl.E10, b"7.7", b"stationer"]
    planted = []
    for unit_max in UNIT_SIZES:
        for j, b in enumerate(unit_borders(LONG_DOC, unit_max)):
            t = across[j % len(across)]
            if j % 40 == 7:
                t = pl.T300
            k = 1 + j % (len(t) - 1)                     # bytes in front of the border
            body[b - k:b - k + len(t)] = t
            planted.append((b, b - k, t))
    docs = _ordinary(rng, 20) + [bytes(body)] + _ordinary(rng, 20)
    return Case("long_doc", docs, b"", b""), planted


def _second_walk():
    rng = _rng(5)
    dense = (b"nationals" * 260)[:2300]                  # more than 1 000 entries in one unit
    docs = _ordinary(rng, 20) + [dense] + _ordinary(rng, 17) + [dense, b""] + _ordinary(rng, 12)
    return Case("second_walk", docs, b"", b"")


@functools.lru_cache(maxsize=None)
def cases():
    c = [_pairs()] + [_empty_run(n) for n in LEADS] + [_blob_end(), _long_doc()[0], _second_walk()]
    return {x.name: x for x in c}


def long_doc_planted():
    return _long_doc()[1]


# ---- expectations: the bare documents, doc_off[0] == 0 ---------------------------------------------------------------------------
EXPRESSIONS = pl.expressions(pl.PRESENCE)


@functools.lru_cache(maxsize=None)
def _oracle():
    o = Oracle(TERMS, POS_START)
    o.set_expressions(list(EXPRESSIONS), True)
    return o


@functools.lru_cache(maxsize=None)
def expected_csr(name, fold):
    blob, off = pack_strings(cases()[name].docs)
    got = _oracle().scan(blob, off, fold=fold)
    for a in got:
        a.setflags(write=False)
    return got


@functools.lru_cache(maxsize=None)
def expected_rows(name, fold):
    blob, off = pack_strings(cases()[name].docs)
    rows = _oracle().process(blob, off, fold=fold)
    rows.setflags(write=False)
    return rows


def placed(name, at=0):
    """-> (buffer, doc_off, text start): placement.place -- lead bytes in front of doc_off[0], the tail in the 64 bytes of slack"""
    c = cases()[name]
    return pl.place(c.docs, c.lead, c.tail, at)
