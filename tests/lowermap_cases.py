"""Inputs and the reference shared by tests/test_lowermap_host.py (the host walk) and tests/test_gpu_lowermap.py (the kernels):
spans of the lower-case form of a batch mapped back to the source text (gft_map_spans_to_source_device).

The reference cuts a document into Go's runes with a sequential decoder written here -- independent of the 16-byte piece code --,
takes every rune's lower-case form from gft_debug_lower_rune (proven equal to gft_to_lower for every code point by
tests/test_tolower_host.py), accumulates (a_i, sl_i, b_i, ll_i) and applies the rule of include/gft.h: a lowered span (start, len)
becomes [a_p, a_q + sl_q), p / q the runes whose lowered bytes hold byte start / start + len - 1; len == 0 gives (a_p, 0), at the
lowered end (len(S), 0); start + len > B is refused."""
import collections
import functools
import random
import re

import numpy as np

import tolower_cases as TC
from gofindthem_amd import _lib
from gofindthem_amd.engine import lowermap_shape

_ASCII_RUN = re.compile(rb"[\x00-\x7f]+")

Runes = collections.namedtuple("Runes", "a sl b ll lowered n")     # numpy int64 arrays per rune, the lowered bytes, len(S)


@functools.lru_cache(maxsize=None)
def _lower_cp(cp):
    return chr(_lib.load().gft_debug_lower_rune(cp)).encode()


def _decode(s, i):
    """utf8.DecodeRune at s[i:] -> (code point or None for one invalid byte, bytes taken)"""
    b0, n = s[i], len(s)

    def cont(k, lo=0x80, hi=0xBF):
        return i + k < n and lo <= s[i + k] <= hi
    if 0xC2 <= b0 <= 0xDF:
        if cont(1):
            return (b0 & 0x1F) << 6 | (s[i + 1] & 0x3F), 2
    elif 0xE0 <= b0 <= 0xEF:
        lo, hi = (0xA0 if b0 == 0xE0 else 0x80), (0x9F if b0 == 0xED else 0xBF)
        if cont(1, lo, hi) and cont(2):
            return (b0 & 0x0F) << 12 | (s[i + 1] & 0x3F) << 6 | (s[i + 2] & 0x3F), 3
    elif 0xF0 <= b0 <= 0xF4:
        lo, hi = (0x90 if b0 == 0xF0 else 0x80), (0x8F if b0 == 0xF4 else 0xBF)
        if cont(1, lo, hi) and cont(2) and cont(3):
            return (b0 & 0x07) << 18 | (s[i + 1] & 0x3F) << 12 | (s[i + 2] & 0x3F) << 6 | (s[i + 3] & 0x3F), 4
    return None, 1


@functools.lru_cache(maxsize=None)
def runes(doc):
    """the runes of one document (bytes), in order"""
    a, sl, ll, low = [], [], [], []
    i, n = 0, len(doc)
    while i < n:
        m = _ASCII_RUN.match(doc, i)
        if m:
            k = m.end() - i
            a.append(np.arange(i, i + k)); sl.append(np.ones(k, np.int64)); ll.append(np.ones(k, np.int64))
            low.append(m.group().lower())
            i += k
            continue
        cp, k = _decode(doc, i)
        out = b"\xef\xbf\xbd" if cp is None else _lower_cp(cp)
        a.append(np.array([i])); sl.append(np.array([k])); ll.append(np.array([len(out)]))
        low.append(out)
        i += k
    cat = lambda xs: np.concatenate(xs).astype(np.int64) if xs else np.zeros(0, np.int64)   # noqa: E731
    a, sl, ll = cat(a), cat(sl), cat(ll)
    b = np.concatenate([[0], np.cumsum(ll)[:-1]]).astype(np.int64) if ll.size else ll
    return Runes(a, sl, b, ll, b"".join(low), n)


def lowered_len(doc):
    return len(runes(doc).lowered)


def map_spans(doc, start, length):
    """the rule over arrays of lowered spans of one document -> (source start, source len) int64 arrays; None: some span is refused"""
    r = runes(doc)
    start, length = np.asarray(start, np.int64), np.asarray(length, np.int64)
    B = len(r.lowered)
    if start.size == 0:
        return start.copy(), length.copy()
    if ((start + length) > B).any():
        return None
    rune_of = np.repeat(np.arange(r.a.size), r.ll)                  # [B]: the rune that holds a lowered byte
    at_end = start == B
    p = rune_of[np.where(at_end, 0, start)] if B else np.zeros(start.size, np.int64)
    q = rune_of[np.where(length > 0, start + length - 1, 0)] if B else p
    a = r.a[p] if B else np.zeros(start.size, np.int64)
    s_start = np.where(at_end, r.n, a)
    s_len = np.where(length > 0, (r.a[q] + r.sl[q] - a) if B else 0, 0)
    return s_start, s_len


FULL = 0xFFFFFFFF
# wrong readings of the span base that only span_off[0] != 0 tells apart: the mapped span written at k instead of s0 + k; the limit
# of gft_map_spans_limit taken as a count behind s0 instead of an index into the caller's arrays
BASE_MUTANTS = ("mapped_at_k", "limit_relative")


def expected(docs, spans, span_lead=0, span_tail=0, limit=None, mutant=None):
    """spans: per document a (start, length) pair of arrays -> (span_off u64, start u32, len u32) mapped, or None when refused.
    span_lead / span_tail: the batch as flat(spans, span_lead, span_tail) hands it over; the arrays are stated at the caller's
    indexes, and an entry outside [span_off[0], span_off[n_docs]) keeps what flat() put there.  limit: only the spans at the
    caller's indexes below it are mapped (gft_map_spans_limit); the others keep their lowered values and are not judged"""
    so, st, ln = flat(spans, span_lead, span_tail)
    s0, end = int(so[0]), int(so[-1])
    if limit is not None:
        end = min(end, s0 + limit) if mutant == "limit_relative" else min(end, max(limit, s0))
    new_st, new_ln = st.copy(), ln.copy()
    for d, (doc, (s, n)) in enumerate(zip(docs, spans)):
        lo = int(so[d])
        k = max(0, min(len(s), end - lo))                           # the spans of this document below the limit
        got = map_spans(doc, np.asarray(s)[:k], np.asarray(n)[:k])
        if got is None:
            return None
        at = lo - s0 if mutant == "mapped_at_k" else lo
        new_st[at:at + k], new_ln[at:at + k] = got[0].astype(np.uint32), got[1].astype(np.uint32)
    return so, new_st, new_ln


def flat(spans, span_lead=0, span_tail=0):
    """the lowered spans as the arrays the calls take: (span_off u64 [n + 1], start u32, len u32).  span_lead / span_tail: entries in
    front of the batch's spans (span_off[0] = span_lead) and behind them; they hold FULL, FULL -- a span the call would refuse if
    it read it"""
    so = np.full(len(spans) + 1, span_lead, np.uint64)
    if spans:
        so[1:] = span_lead + np.cumsum([len(s) for s, _ in spans], dtype=np.uint64)
    pad = lambda k: [np.full(k, FULL, np.int64)]                    # noqa: E731
    cat = lambda xs: np.concatenate([np.asarray(x, np.int64) for x in xs]).astype(np.uint32)   # noqa: E731
    return so, cat(pad(span_lead) + [s for s, _ in spans] + pad(span_tail)), cat(pad(span_lead) + [n for _, n in spans] + pad(span_tail))


def base_docs():
    """a small batch whose spans move and change length under the map: what assert_not_vacuous and the tests of runs use"""
    docs = ["CAFÉ İK one".encode(), b"", "İİ two Ⱥ Ⱥ".encode(), b"plain", b"three \xff\xff K".replace(b"K", "\u212a".encode()), "Ⱥ".encode() * 9]
    return docs, [every_byte(d, n_random=12, seed=i) if i != 3 else (np.zeros(0, np.int64), np.zeros(0, np.int64)) for i, d in enumerate(docs)]


def assert_not_vacuous(span_lead=1, span_tail=1):
    """the base mutants are the reference itself with span_off[0] == 0 -- that is the gap -- and differ behind span_lead entries, on
    the batch of base_docs(); the limit at every index from 0 to past the end.  Returns {mutant: the (span_lead, limit) that catch it}"""
    docs, spans = base_docs()
    n = sum(len(s) for s, _ in spans)
    told = {}
    for m in BASE_MUTANTS:
        limits = [None] if m == "mapped_at_k" else [0, 1, n // 2, n, n + 1, n + span_lead, n + span_lead + 5]
        differs = lambda lead, tail, lim: any(not np.array_equal(a, b) for a, b in zip(expected(docs, spans, lead, tail, lim, m),   # noqa: E731
                                                                                       expected(docs, spans, lead, tail, lim)))
        blind = [lim for lim in limits if differs(0, 0, lim)]
        assert not blind, "the mutant %r shows without a span base at the limits %r" % (m, blind)
        told[m] = [(span_lead, lim) for lim in limits if differs(span_lead, span_tail, lim)]
        assert told[m], "a span base of %d does not tell the mutant %r from the contract" % (span_lead, m)
    return told


def every_byte(doc, n_random=200, seed=1):
    """every single-byte span of the lowered document, the whole-document span, and n_random seeded (start, len)"""
    B = lowered_len(doc)
    rng = random.Random(seed * 1000003 + B)
    s = list(range(B)) + [0]
    n = [1] * B + [B]
    for _ in range(n_random):
        x = rng.randint(0, B)
        s.append(x); n.append(rng.randint(0, min(B - x, 40)))
    return np.asarray(s, np.int64), np.asarray(n, np.int64)


def around(doc, src_at, reach=8):
    """the single-byte spans within `reach` lowered bytes of the rune that begins at source byte src_at"""
    r = runes(doc)
    i = int(np.searchsorted(r.a, src_at))
    assert r.a[i] == src_at
    lo, hi = max(0, int(r.b[i]) - reach), min(len(r.lowered), int(r.b[i] + r.ll[i]) + reach)
    s = np.arange(lo, hi, dtype=np.int64)
    return s, np.ones(s.size, np.int64)


def border_runes():
    return [chr(cp).encode() for cp in TC.LENGTH_CHANGERS] + [TC.RUNES[k].encode() for k in (2, 3, 4)] + list(TC.INVALID)


def borders():
    """name -> (source offset of the border, document length or None): the piece, the trip and the unit figure of
    gft_debug_lowermap_shape, and -- the lower kernels cut a document of n > unit bytes into equal slices -- the cut between the
    two units of a document of unit + 108 bytes"""
    piece, trip, unit, _ = lowermap_shape()
    n = unit + 108
    return {"piece": (piece, None), "trip": (trip, None), "unit": (unit, None), "unit cut": ((n + 1) // 2, n)}


def border_docs(which=None, every=1):
    """[(document, source offset of the placed rune)]: each rune of border_runes() with its FIRST byte at border - j, j < len"""
    out = []
    for name, (k, total) in borders().items():
        if which is not None and name not in which:
            continue
        for i, r in enumerate(border_runes()):
            if i % every:
                continue
            for j in range(len(r)):
                d = TC._ascii(k - j, k + j) + r + TC._ascii(40, i)
                if total is not None:
                    d += TC._ascii(total - len(d), 7)
                out.append((d, k - j))
    return out


def fold_safe_docs():
    return [b"plain ASCII with CAPITALS 0123", "café ÿ naïve ça".encode(), b"", b"x", ("é" * 700).encode(), TC._ascii(9000, 3)]
