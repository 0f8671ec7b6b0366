"""Batches for the top of k_scan5's unit loop (test infrastructure: numpy only, no GPU, no tests in here).  A wave requests its
unit's first bytes, takes its next work item, and loads that unit's record -- unconditionally, at an index clamped to the last
unit -- and the blob offsets of the record's document; whether there is a next unit is asked by the loop's condition.  What such
a top can get wrong is the LAST unit of a wave (the clamped record is some other unit's: nothing of it may be scanned or
flushed), waves that never get a unit, the order of a unit's own first loads, and the next unit's document when it is the
current one.  One workgroup (schema_scale.ONE_CU) takes all units, so the counts below are units per workgroup of 16 waves.

    one            a batch of one unit
    few            5 units: eleven waves of the workgroup never get one
    n15 .. n49     15, 16, 17, 31, 33, 47 and 49 units: 16 k - 1, 16 k and 16 k + 1
    last_empty     the last document is empty (the last unit owns no byte)
    first_empty    the first one is
    doc8193        a document of 8 193 bytes between short ones: two units, the second begins at lo > 0 and a wave's next unit
    doc16385       lies in the document it is scanning; 16 385 bytes: three units
    blob_end       the last document ends with a keyword on the blob's last byte; the slack behind it completes longer ones
    lead0 .. lead3 the first document starts at bytes 0 to 3 of the text buffer, keywords in its first bytes: each lane's history
                   word is gathered byte by byte; the lead bytes would complete a cut keyword
    pool           (pool_case) more matches than the engine's match pool holds: the batch is scanned a second time

Every case runs under a dictionary of 30 byte classes (TERMS_SMALL: the short terms through the direct table) and one of 51
(TERMS_LARGE: the group-indexed tables); the documents are ASCII and spell keywords of both.  Expectations come from
oracle.pyoracle on the bare documents."""
import collections
import functools

import numpy as np

import placement as pl
import unit_boundaries as ub
from oracle.pyoracle import POS_START, Oracle, pack_strings

WAVES = 16
COUNTS = (15, 16, 17, 31, 33, 47, 49)
LEADS = (0, 1, 2, 3)
LEAD = b"zxq"                       # its last 1, 2 or 3 bytes in front of "7.7 ...": "q7", "xq" + "7"; "zxq" ends in front of doc_off[0]
LONG_DOCS = (8193, 16385)
_SMALL_BYTES = frozenset(b"abcdefghijklmnopqrstuvwxyz 7.")
LONG_TERM = pl._word(np.random.default_rng(20261021), 280)
TERMS_SMALL = [t for t in pl.TERMS_ASCII if set(t) <= _SMALL_BYTES] + [LONG_TERM]
TERMS_LARGE = pl.TERMS_MIXED + [LONG_TERM]
DICTIONARIES = {"small": TERMS_SMALL, "large": TERMS_LARGE}

Case = collections.namedtuple("Case", "name docs lead tail")


def classes(terms):
    """byte classes of a dictionary: its distinct bytes and one more for every other byte"""
    return len({b for t in terms for b in t}) + 1


def _rng(*salt):
    return np.random.default_rng([20261021, *salt])


def _text(rng, n):
    """n bytes that spell keywords of TERMS_SMALL (tiny documents start with short keywords)"""
    if n <= 5:
        return (b"q7.7 ", b"zxq7 ", b"kjq7.", b"7.7q ", b"wxyz ")[int(rng.integers(5))][:n]
    return pl._dense(rng, TERMS_SMALL, n + 40)[:n]


def _ordinary(rng, n):
    return [_text(rng, int(m)) for m in rng.integers(1, 400, n)]


def _count(n):
    return Case("n%d" % n if n > 5 else ("one" if n == 1 else "few"), _ordinary(_rng(1, n), n), b"", b"")


def _long_doc(n):
    """keywords back to back and the 280-byte one now and then: some keyword lies across every unit border, whatever the unit"""
    rng = _rng(2, n)
    body = bytearray((b"nationals" * (n // 9 + 1))[:n])
    for at in range(700, n - 300, 1500):
        body[at:at + len(LONG_TERM)] = LONG_TERM
    docs = _ordinary(rng, 9) + [bytes(body)] + _ordinary(rng, 9)
    return Case("doc%d" % n, docs, b"", b"")


def _lead(k):
    rng = _rng(3)
    first = b"7.7 q7 " + pl.T10 + b" " + _text(rng, 300)   # "7" at offset 0, "7.7" at 0 .. 2
    return Case("lead%d" % k, [first] + _ordinary(rng, 20), LEAD[len(LEAD) - k:], b"")


@functools.lru_cache(maxsize=None)
def cases():
    rng = _rng(4)
    blob_end = ub.cases()["blob_end"]
    c = [_count(1), _count(5)] + [_count(n) for n in COUNTS]
    c += [Case("last_empty", _ordinary(rng, 20) + [b""], b"", b""), Case("first_empty", [b""] + _ordinary(rng, 20), b"", b"")]
    c += [_long_doc(n) for n in LONG_DOCS]
    c += [Case("blob_end", list(blob_end.docs), b"", blob_end.tail)]
    c += [_lead(k) for k in LEADS]
    return {x.name: x for x in c}


# ---- expectations: the bare documents, doc_off[0] == 0 ---------------------------------------------------------------------------
def _q(t):
    return '"%s"' % t.decode("utf-8")


@functools.lru_cache(maxsize=None)
def expressions():
    """one UNIT per keyword of TERMS_SMALL (both dictionaries hold them) and a few AND / OR / NOT: no position is read"""
    e = [_q(t) for t in sorted(TERMS_SMALL)]
    e += ['%s and %s' % (_q(pl.T10), _q(pl.E10)), 'not %s' % _q(pl.T10), '%s and not %s' % (_q(b"q"), _q(b"zx")),
          '%s and %s and %s' % (_q(b"nation"), _q(b"nations"), _q(b"national")), '%s or %s or %s' % (_q(b"kjq"), _q(b"wxyz"), _q(b"7.7")),
          'not (%s or %s)' % (_q(LONG_TERM), _q(pl.E10)), '%s and not (%s and %s)' % (_q(b"q7"), _q(b"zxq"), _q(b"alpha"))]
    return tuple(e)


@functools.lru_cache(maxsize=None)
def oracle(which):
    o = Oracle(DICTIONARIES[which], POS_START)
    o.set_expressions(list(expressions()), True)
    return o


@functools.lru_cache(maxsize=None)
def expected_csr(name, which, fold):
    blob, off = pack_strings(cases()[name].docs)
    got = oracle(which).scan(blob, off, fold=fold)
    for a in got:
        a.setflags(write=False)
    return got


@functools.lru_cache(maxsize=None)
def expected_rows(name, which, fold):
    blob, off = pack_strings(cases()[name].docs)
    rows = oracle(which).process(blob, off, fold=fold)
    rows.setflags(write=False)
    return rows


def placed(name):
    """-> (buffer, doc_off, text start): the text pointer is the buffer's first byte, doc_off[0] == len(lead)"""
    c = cases()[name]
    return pl.place(c.docs, c.lead, c.tail, 0)


# ---- more matches than the pool holds ------------------------------------------------------------------------------------------
POOL_MIN = 1 << 20                  # entries of the smallest match pool (gft_pipeline.cpp)
POOL_DOCS = 720


@functools.lru_cache(maxsize=None)
def pool_case(fold):
    """-> (documents, expected rows, entries a presence-only scan writes at least): three dense documents of about 4 000 bytes,
    repeated -- "nationals" back to back is four keywords of four bytes and more per nine bytes, and every occurrence of such a
    keyword is a pool entry.  The expectation is the oracle's on the three, repeated"""
    three = [(b"nationals" * 450)[:n] for n in (4000, 3999, 4001)]
    blob, off = pack_strings(three)
    o = oracle("small")
    rows = o.process(blob, off, fold=fold)
    long_ids = [i for i, t in enumerate(sorted(set(TERMS_SMALL))) if len(t) >= 4]
    m_off, term, _ = o.scan(blob, off, fold=fold)
    per_doc = [int(np.isin(term[int(m_off[d]):int(m_off[d + 1])], long_ids).sum()) for d in range(3)]
    reps = POOL_DOCS // 3 + 1
    docs = (three * reps)[:POOL_DOCS]
    want = np.tile(rows, (reps, 1))[:POOL_DOCS]
    want.setflags(write=False)
    return docs, want, sum((per_doc * reps)[:POOL_DOCS])
