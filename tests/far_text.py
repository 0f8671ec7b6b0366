"""Text past 4 GiB (test infrastructure: numpy only, no GPU, nothing of the product loaded at import): `filler`, a byte per 64-bit
position that depends on every bit of the position; the border placements that put a fixed case across position 2^32 of one
allocation; the long batch -- islands of fixed cases between documents of just under 1 GiB of filler, laid out so that input
position 2^32 falls inside a span in the middle of an island --; and the sparse references of the document-independent calls over
that batch, which never materialise a long document: an output blob is a list of segments ("text", src_lo, src_hi) /
("bytes", literal), every array output is computed in Python integers.  An island's answer is the existing dense reference's
(replace.expected, mark.expected, excerpts.expected, spans.redact_reference's slicing, route_docs.buckets_of, tolower_cases); a long
document's answer is computed from its length and its planted hits alone, which is valid because the filler is ASCII without
upper-case letters and holds no byte of a planted hit; the scan, the solver, the hit spans, the map and the word filter are answered
on a compressed twin of it (twin()).  The same code at a scaled-down size (long documents of three tiles) is
compared with the dense references over the whole batch by test_far_text_host.py.  No tests in here."""
import bisect
import collections
import functools

import numpy as np

B = 1 << 32
SLACK = 64
POISON = 0xEE
WINDOW = 1 << 20                                    # the largest placed text of layer A; the allocation is B + WINDOW + SLACK bytes
TILE = 4096

# ---- the filler ------------------------------------------------------------------------------------------------------------------
GOLDEN = 0x9E3779B97F4A7C15
GOLDEN_I64 = GOLDEN - (1 << 64)                     # the same bits as a signed 64-bit integer
# 32 bytes: digits and punctuation -- no letter (every keyword used at scale is letters), no byte of the markers, the replacements
# or the mask of layer B, no newline, nothing >= 0x80, no upper case
ALPHABET = b"0123456789 .,;:-_()=+&%$#@!?~^|`"
assert len(ALPHABET) == len(set(ALPHABET)) == 32 and max(ALPHABET) < 0x80 and b"\n" not in ALPHABET
_TABLE = np.frombuffer(ALPHABET, np.uint8)


def top_byte(pos):
    """the top byte of pos * GOLDEN in wrapping 64-bit arithmetic (numpy int64 array or scalar): the filler's raw form"""
    with np.errstate(over="ignore"):
        p = np.asarray(pos, dtype=np.int64) * np.int64(GOLDEN_I64)
    return ((p >> 56) & 0xFF).astype(np.uint8)                     # (the shift is arithmetic: mask after it)


def filler(pos):
    """the byte at 64-bit position `pos`: the top five bits of pos * GOLDEN through ALPHABET"""
    return _TABLE[top_byte(pos) >> 3]


def filler_range(lo, hi):
    return filler(np.arange(lo, hi, dtype=np.int64))


def top_byte_torch(pos):
    """top_byte on a torch int64 tensor (any device): int64 multiplication wraps there too"""
    return ((pos * GOLDEN_I64) >> 56) & 0xFF


def filler_torch(pos, table):
    """filler on a torch int64 tensor; table: ALPHABET as a uint8 tensor on pos's device"""
    return table[top_byte_torch(pos) >> 3]


# ---- layer A: a fixed case across 2^32 ---------------------------------------------------------------------------------------------
BORDER_NAMES = ("B-size-1", "B-size", "B-size/2", "B-17", "B-1", "B", "B+1")


def border_placements(size):
    """[(name, at)]: where the placed text -- `size` bytes, its lead bytes included -- begins in the allocation.  doc_off[0] is
    at + lead; the text pointer is the allocation's base, so at % 16 varies the residue as well.  "B-size-1": the slack crosses B;
    "B-size": the text ends exactly at B"""
    return list(zip(BORDER_NAMES, (B - size - 1, B - size, B - size // 2, B - 17, B - 1, B, B + 1)))


def fits(size):
    """the stated rule by which layer A leaves a case out: its text, lead included, does not fit the window behind B + 1"""
    return size < WINDOW


def strictly_inside(at, intervals):
    """does B lie strictly inside one of the half-open intervals [lo, hi) of the placed text (positions from its first byte)?"""
    return any(at + lo < B < at + hi for lo, hi in intervals)


# ---- layer B: the long batch -------------------------------------------------------------------------------------------------------
# body: an island document's bytes, None: a long document; plants: [(position in the document, bytes)] written over a long one's filler
Doc = collections.namedtuple("Doc", "island body length spans plants")
# the planted hits: letters the filler lacks; HIT in mixed case, so that lowering changes it and only a folding scan finds it
HIT = b"GoFindThemFar"
_LETTERS = b"bdfghjklmpvw"


def _word(n, salt):
    rng = np.random.default_rng([20261020, salt])
    return bytes(_LETTERS[int(i)] for i in rng.integers(0, len(_LETTERS), n))


# the dictionary of layer B: eight lower-case keywords, one per length class of placement.length_classes and two more
K2, K3, K4, K6, K13, K26, K33, K300 = b"kq", b"zxq", b"wxyz", HIT[:6].lower(), HIT.lower(), _word(26, 1), _word(33, 2), _word(300, 3)
TERMS = [K2, K3, K4, K6, K13, K26, K33, K300]
_Q = lambda t: '"%s"' % t.decode()                                   # noqa: E731
# a single keyword, an `and`, a `not`, an `inord` that holds in a long document (wxyz stands in front of zxq), one that does not, and
# one that holds only under the fold (behind K33 stands HIT alone, in mixed case)
EXPRS = (_Q(K2), "%s and %s" % (_Q(K13), _Q(K4)), "not %s" % _Q(K3), "inord(%s and %s)" % (_Q(K4), _Q(K3)), "inord(%s and %s)" % (_Q(K33), _Q(K26)),
         "%s or %s" % (_Q(K300), _Q(K6)), "%s and not %s" % (_Q(K26), _Q(K300)), "inord(%s and %s)" % (_Q(K33), _Q(K13)))
OPEN, CLOSE = b"<em>", b"</em>"
REPS = [b"", b"[LongerThanTheRunItReplaces]", b"<rr>", b"{three}"]    # one empty, one longer than any planted run
KEY_REP = [1, 0, 3, 2, 1, 0]                                            # a keyed table: key -> replacement
MASK = 0x2A
BEFORE, AFTER = 40, 24
N_COLS = 40
LONG_4 = 5 * (1 << 27) - 77                                         # 640 MiB less a few: the batch is about 4.6 GiB


def _islands():
    """six document lists of existing fixed cases, with their spans (start, len, key): replace.py's, whose documents and spans are
    mark.py's; island 4 is "straddle_tile", 8 292 bytes with a span over its first tile border"""
    import replace as R
    by = {c.name: c for c in R.fixed_cases()}
    names = ("touch_across_docs", "empty_docs", "second_doc_ranks", "text_residue_5", "straddle_tile", "many_runs_in_tile")
    out = []
    for i, n in enumerate(names):
        c = by[n]
        spans = [[(a, ln, (k + j + i) % len(KEY_REP)) for j, (a, ln, k) in enumerate(sp)] for sp in c.spans]
        docs = list(c.docs)
        if n == "empty_docs":                                       # a document that leaves ASCII, grows and shrinks when lowered
            # (... with keywords behind the runes that change length: their spans in the lowered text move under the map)
            docs.append("CAFÉ İ kq İİ WXYZ Ⱥ ẞ gofindthemfar straße Ⱥ zxq".encode())
            spans.append([])
        out.append((n, docs, spans))
    return out


class LongBatch:
    """island_0, long_0, island_1, ..., long_4, island_5.  long_len None: the real thing -- long_0 .. long_3 of just under 1 GiB,
    chosen so that position B is byte 4 098 of island 4, inside its span (4 094, 8), long_4 of LONG_4 bytes --; a number: every long
    document of that many bytes (the host test's scaled-down twin; `cross` is then a position inside the same span)"""

    def __init__(self, long_len=None):
        self.islands = _islands()
        isl = [sum(len(d) for d in docs) for _, docs, _ in self.islands]
        target = TILE + 2                                           # of island 4: inside its span [4 094, 4 102)
        if long_len is None:
            lens = [(1 << 30) - 1111, (1 << 30) - 2223, (1 << 30) - 3]
            lens.append(B - target - sum(isl[:4]) - sum(lens))
            lens.append(LONG_4)
            assert all((1 << 30) - (1 << 20) < x < 1 << 30 for x in lens[:4])
        else:
            lens = [long_len + 3 * k for k in range(5)]
        self.docs, self.long_at, self.island_at = [], [], []
        for k, (name, docs, spans) in enumerate(self.islands):
            self.island_at.append(len(self.docs))
            self.docs += [Doc(k, d, len(d), s, None) for d, s in zip(docs, spans)]
            if k < 5:
                self.long_at.append(len(self.docs))
                self.docs.append(Doc(None, None, lens[k], None, None))
        self.off = [0]
        for d in self.docs:
            self.off.append(self.off[-1] + d.length)
        self.total = self.off[-1]
        self.cross = self.off[self.island_at[4]] + target
        assert long_len is not None or self.cross == B
        # the hits of a long document: in its first 64 bytes (two that touch, and an empty span), across a 4 KiB border of the batch
        # and across one of the document in its middle, and in its last 64 bytes
        # (a whole word " kq ", and "_zxq", which the word filter drops)
        for i in self.long_at:
            lo, L = self.off[i], self.docs[i].length
            h = len(HIT)
            mid = lo + L // 2
            bb = mid - mid % TILE - 150 - lo                        # K300 lies across a multiple of 4 096 of the batch's positions
            db = (L // 2 + TILE) - (L // 2) % TILE - 9              # ... K26 across one of the document's
            if db < bb + 400:
                db += TILE
            plants = [(5, HIT), (5 + h, K13), (44, K4), (49, b"_" + K3), (56, b" " + K2 + b" "), (bb, K300), (db, K26), (L - 62, K33), (L - 20, HIT)]
            spans = [(5, h, 2), (5 + h, h, 0), (40, 0, 4), (44, 4, 1), (50, 3, 3), (57, 2, 5), (bb, 300, 1), (db, 26, 3), (L - 62, 33, 0), (L - 20, h, 5)]
            assert 64 < bb and bb + 300 < db and db + 26 < L - 62, (L, bb, db)
            assert (lo + bb) // TILE != (lo + bb + 299) // TILE and db // TILE != (db + 25) // TILE
            assert all(a + len(b) <= c for (a, b), (c, _) in zip(plants, plants[1:])) and plants[-1][0] + h <= L
            self.docs[i] = self.docs[i]._replace(spans=spans, plants=plants)
        self.n = len(self.docs)

    # -- the input --
    def hits(self, i):
        """[(position in the batch, bytes)] planted in long document i"""
        return [(self.off[i] + a, b) for a, b in self.docs[i].plants]

    def read(self, lo, hi):
        """the batch's bytes [lo, hi) as a uint8 array, for short ranges: islands from their documents, long documents from filler
        and hits"""
        out = filler_range(lo, hi)
        d = bisect.bisect_right(self.off, lo) - 1
        while d < self.n and self.off[d] < hi:
            doc, a = self.docs[d], self.off[d]
            if doc.body is not None:
                s, e = max(lo, a), min(hi, a + doc.length)
                if e > s:
                    out[s - lo:e - lo] = np.frombuffer(doc.body, np.uint8)[s - a:e - a]
            else:
                for p, h in self.hits(d):
                    s, e = max(lo, p), min(hi, p + len(h))
                    if e > s:
                        out[s - lo:e - lo] = np.frombuffer(h, np.uint8)[s - p:e - p]
            d += 1
        return out

    def dense(self):
        """the whole batch's bytes (the scaled-down twin only)"""
        assert self.total < 1 << 24
        return self.read(0, self.total).tobytes()

    def bodies(self):
        text = self.dense()
        return [text[self.off[d]:self.off[d + 1]] for d in range(self.n)]

    def span_arrays(self):
        """(span_off, start, len, key) as lists"""
        so, st, ln, ky = [0], [], [], []
        for d in self.docs:
            for a, n, k in d.spans:
                st.append(a)
                ln.append(n)
                ky.append(k)
            so.append(len(st))
        return so, st, ln, ky

    def island_docs(self, k):
        a = self.island_at[k]
        return range(a, a + len(self.islands[k][1]))


@functools.lru_cache(maxsize=None)
def long_batch(long_len=None):
    return LongBatch(long_len)


# ---- sparse references ---------------------------------------------------------------------------------------------------------------
def seg_len(s):
    return s[2] - s[1] if s[0] == "text" else len(s[1])


def _text(segs, lo, hi):
    if hi > lo:
        segs.append(("text", lo, hi))


def _bytes(segs, b):
    if b:
        segs.append(("bytes", bytes(b)))


def _runs(spans, ids=None):
    """the connected components of the union of [start, start + len), touching ones united: [S, E, smallest id]"""
    comps = []
    for lo, hi, k in sorted((a, a + n, k) for k, (a, n, _) in enumerate(spans)):
        if comps and lo <= comps[-1][1]:
            comps[-1][1] = max(comps[-1][1], hi)
            comps[-1][2].append(k)
        else:
            comps.append([lo, hi, [k]])
    return [[S, E, min(ids[k] for k in ks) if ids else 0] for S, E, ks in comps]


def _per_island(lb, fn):
    """{first document of island k: fn(k, docs, spans)}"""
    return {lb.island_at[k]: fn(k, docs, spans) for k, (_, docs, spans) in enumerate(lb.islands)}


def sparse_mark(lb):
    """-> {"segs", "total", "n_runs", "out_off", "span_new", "doc_run_off"}"""
    import mark as M
    dense = _per_island(lb, lambda k, docs, spans: M.expected(M.Case("island", docs, [[s[:2] for s in sp] for sp in spans], OPEN, CLOSE)))
    segs, out_off, span_new, dro = [], [0], [], [0]
    d = 0
    while d < lb.n:
        doc, lo = lb.docs[d], lb.off[d]
        if doc.body is not None:
            w, n = dense[d], len(lb.islands[doc.island][1])
            _bytes(segs, w["out"])
            base = out_off[-1]
            out_off += [base + v for v in w["out_off"][1:]]
            span_new += w["span_new"]
            dro += [dro[-1] + v for v in w["doc_run_off"][1:]]
            d += n
            continue
        comps = _runs(doc.spans)
        firsts, pos = [S for S, _, _ in comps], 0
        for S, E, _ in comps:
            _text(segs, lo + pos, lo + S)
            _bytes(segs, OPEN)
            _text(segs, lo + S, lo + E)
            _bytes(segs, CLOSE)
            pos = E
        _text(segs, lo + pos, lo + doc.length)
        for a, n, _ in doc.spans:
            r = bisect.bisect_right(firsts, a) - 1
            span_new.append(a + (r + 1) * len(OPEN) + r * len(CLOSE))
        out_off.append(out_off[-1] + doc.length + len(comps) * (len(OPEN) + len(CLOSE)))
        dro.append(dro[-1] + len(comps))
        d += 1
    return {"segs": segs, "total": out_off[-1], "n_runs": dro[-1], "out_off": out_off, "span_new": span_new, "doc_run_off": dro}


def sparse_replace(lb):
    """-> {"segs", "total", "n_runs", "out_off", "doc_run_off", "run_new", "run_len", "run_rep"}"""
    import replace as R
    dense = _per_island(lb, lambda k, docs, spans: R.expected(R.Case("island", docs, spans, REPS, KEY_REP)))
    segs, out_off, dro, run_new, run_len, run_rep = [], [0], [0], [], [], []
    d = 0
    while d < lb.n:
        doc, lo = lb.docs[d], lb.off[d]
        if doc.body is not None:
            w, n = dense[d], len(lb.islands[doc.island][1])
            _bytes(segs, w["out"])
            base = out_off[-1]
            out_off += [base + v for v in w["out_off"][1:]]
            dro += [dro[-1] + v for v in w["doc_run_off"][1:]]
            run_new += w["run_new"]
            run_len += w["run_len"]
            run_rep += w["run_rep"]
            d += n
            continue
        comps = _runs(doc.spans, [KEY_REP[k] for _, _, k in doc.spans])
        pos, cut, put = 0, 0, 0
        for S, E, rid in comps:
            _text(segs, lo + pos, lo + S)
            _bytes(segs, REPS[rid])
            run_new.append(S - cut + put)
            run_len.append(len(REPS[rid]))
            run_rep.append(rid)
            cut += E - S
            put += len(REPS[rid])
            pos = E
        _text(segs, lo + pos, lo + doc.length)
        out_off.append(out_off[-1] + doc.length - cut + put)
        dro.append(dro[-1] + len(comps))
        d += 1
    return {"segs": segs, "total": out_off[-1], "n_runs": dro[-1], "out_off": out_off, "doc_run_off": dro, "run_new": run_new, "run_len": run_len,
            "run_rep": run_rep}


def sparse_redact(lb):
    """the masked batch, in place: the text itself but for MASK over every span -> {"segs", "total"}"""
    segs = []
    for d, doc in enumerate(lb.docs):
        lo, pos = lb.off[d], 0
        for S, E, _ in _runs(doc.spans):
            _text(segs, lo + pos, lo + S)
            _bytes(segs, bytes([MASK]) * (E - S))
            pos = E
        _text(segs, lo + pos, lo + doc.length)
    return {"segs": segs, "total": lb.total}


def sparse_excerpt(lb):
    """-> {"segs", "total", "n_exc", "exc_off", "exc_doc", "exc_start", "exc_span_off", "span_rel", "doc_exc_off"}; a long document
    is ASCII, so no window of its snaps to a rune"""
    import excerpts as X
    dense = _per_island(lb, lambda k, docs, spans: X.expected(X.Case("island", docs, [[s[:2] for s in sp] for sp in spans], BEFORE, AFTER, True)))
    so = lb.span_arrays()[0]
    segs, exc_off, exc_doc, exc_start, eso, rel, deo = [], [0], [], [], [], [], [0]
    d = 0
    while d < lb.n:
        doc, lo = lb.docs[d], lb.off[d]
        if doc.body is not None:
            w, n = dense[d], len(lb.islands[doc.island][1])
            _bytes(segs, w["out"])
            exc_off += [exc_off[-1] + v for v in w["exc_off"][1:]]
            exc_doc += [d + v for v in w["exc_doc"]]
            exc_start += w["exc_start"]
            eso += [so[d] + v for v in w["exc_span_off"][:-1]]
            rel += w["span_rel"]
            deo += [deo[-1] + v for v in w["doc_exc_off"][1:]]
            d += n
            continue
        wins = [(max(0, a - BEFORE), min(doc.length, a + n + AFTER)) for a, n, _ in doc.spans]
        comps = []
        for k, (a, b) in enumerate(wins):                           # (the planted spans are listed by position)
            if comps and a <= comps[-1][1]:
                comps[-1][1] = max(comps[-1][1], b)
                comps[-1][2].append(k)
            else:
                comps.append([a, b, [k]])
        assert wins == sorted(wins)
        for S, E, ks in comps:
            _text(segs, lo + S, lo + E)
            exc_off.append(exc_off[-1] + E - S)
            exc_doc.append(d)
            exc_start.append(S)
            eso.append(so[d] + ks[0])
            rel += [doc.spans[k][0] - S for k in ks]
        deo.append(len(exc_doc))
        d += 1
    eso.append(so[-1])
    return {"segs": segs, "total": exc_off[-1], "n_exc": len(exc_doc), "exc_off": exc_off, "exc_doc": exc_doc, "exc_start": exc_start,
            "exc_span_off": eso, "span_rel": rel, "doc_exc_off": deo}


def sparse_lower(lb):
    """-> {"segs", "total", "out_off"}: an island document through tolower_cases.ref_lower, a long document itself but for its hits"""
    import tolower_cases as TC
    segs, out_off = [], [0]
    for d, doc in enumerate(lb.docs):
        lo = lb.off[d]
        if doc.body is not None:
            low = TC.ref_lower(doc.body)
            _bytes(segs, low)
            out_off.append(out_off[-1] + len(low))
            continue
        pos = lo
        for p, h in lb.hits(d):
            _text(segs, pos, p)
            _bytes(segs, h.lower())
            pos = p + len(h)
        _text(segs, pos, lo + doc.length)
        out_off.append(out_off[-1] + doc.length)
    return {"segs": segs, "total": out_off[-1], "out_off": out_off}


ROUTE_MODE, ROUTE_REST = "every", False


def route_rows(lb):
    """(rows uint32 [n, W], masks uint32 [2, W]) over N_COLS columns, tail bits ones: bucket 0 owns column 3, bucket 1 column 37.
    Every long document goes to both buckets but long_1 (bucket 0 only); the island documents by turns to bucket 0, bucket 1,
    both and neither -- so bucket_byte[1] passes 2^32, bucket_byte[2] 2^33, and out_off both"""
    import route_docs as RD
    bits = np.zeros((lb.n, N_COLS), dtype=bool)
    bits[:, 5] = True                                               # a column no bucket owns
    for d, doc in enumerate(lb.docs):
        if doc.body is None:
            k = lb.long_at.index(d)
            bits[d, 3], bits[d, 37] = True, k != 1
        else:
            bits[d, 3], bits[d, 37] = d % 4 in (0, 2), d % 4 in (1, 2)
    m = np.zeros((2, N_COLS), dtype=bool)
    m[0, 3] = m[1, 37] = True
    return RD._pack(bits, N_COLS), RD._pack(m, N_COLS)


def sparse_route(lb):
    """-> {"segs", "total", "out_off", "doc_idx", "bucket_doc", "bucket_byte"}; the members by route_docs.buckets_of, which reads no text"""
    import route_docs as RD
    rows, masks = route_rows(lb)
    segs, out_off, idx, bd, bb = [], [0], [], [0], [0]
    for members in RD.buckets_of(lb.off, rows, N_COLS, masks, ROUTE_MODE, ROUTE_REST, None):
        for d in members:
            _text(segs, lb.off[d], lb.off[d + 1])
            out_off.append(out_off[-1] + lb.docs[d].length)
            idx.append(d)
        bd.append(len(idx))
        bb.append(out_off[-1])
    return {"segs": segs, "total": out_off[-1], "out_off": out_off, "doc_idx": idx, "bucket_doc": bd, "bucket_byte": bb}


# ---- the compressed twin: the scan, the solver, the hit spans and the map over a long document --------------------------------------
REACH = 1024


def twin(lb, d):
    """long document d with every stretch of filler farther than REACH bytes from a planted hit cut out -> (bytes, [(first position
    of a kept range in the twin, the bytes cut in front of it)]).  Valid as a stand-in for the document wherever only keyword
    occurrences count: the filler holds no byte of a keyword, so the twin's match list is the document's but for the positions,
    whose order is unchanged -- a position of the twin becomes one of the document by adding the cut lengths"""
    doc, lo = lb.docs[d], lb.off[d]
    keep = []
    for a, b in doc.plants:
        s, e = max(0, a - REACH), min(doc.length, a + len(b) + REACH)
        if keep and s <= keep[-1][1]:
            keep[-1][1] = max(keep[-1][1], e)
        else:
            keep.append([s, e])
    parts, starts, at = [], [], 0
    for s, e in keep:
        parts.append(lb.read(lo + s, lo + e).tobytes())
        starts.append((at, s - at))
        at += e - s
    return b"".join(parts), starts


def untwin(starts, pos):
    """a position of the twin as a position of the document"""
    i = bisect.bisect_right([t for t, _ in starts], pos) - 1
    return pos + starts[i][1]


@functools.lru_cache(maxsize=None)
def compressed(long_len=None):
    """(documents: the islands' as they are, the long ones' twins; per document the twin's starts, None for an island document)"""
    lb = long_batch(long_len)
    docs, maps = [], []
    for d, doc in enumerate(lb.docs):
        if doc.body is not None:
            docs.append(doc.body)
            maps.append(None)
        else:
            t, st = twin(lb, d)
            docs.append(t)
            maps.append(st)
    return docs, maps


def _back(maps, d, pos):
    return pos if maps[d] is None else untwin(maps[d], pos)


@functools.lru_cache(maxsize=None)
def sparse_scan(pos_end, fold, long_len=None):
    """(match_off, term_id, pos) as lists: long_terms.brute_force over the compressed documents, the positions mapped back"""
    from long_terms import brute_force
    from oracle.pyoracle import POS_END, POS_START
    docs, maps = compressed(long_len)
    mo, ti, po = brute_force(TERMS, docs, POS_END if pos_end else POS_START, fold)
    mo, ti, po = mo.tolist(), ti.tolist(), po.tolist()
    pos = [_back(maps, d, po[m]) for d in range(len(docs)) for m in range(mo[d], mo[d + 1])]
    return mo, ti, pos


def lowered_docs(docs):
    import tolower_cases as TC
    return [TC.ref_lower(d) for d in docs]


@functools.lru_cache(maxsize=None)
def sparse_rows(fold, long_len=None):
    """the oracle's rows of EXPRS over the compressed documents, uint32 [n, 1], tail bits as the oracle leaves them.  fold: the
    finder's case rule over a batch that leaves ASCII -- strings.ToLower document by document, then the lower-case dictionary"""
    from oracle.pyoracle import Oracle, pack_strings
    docs, _ = compressed(long_len)
    o = Oracle(TERMS)
    o.set_expressions(list(EXPRS), True)
    blob, off = pack_strings(lowered_docs(docs) if fold else docs)
    return o.process(blob, off, fold=False)


@functools.lru_cache(maxsize=None)
def sparse_hit_spans(lowered, long_len=None):
    """{"span_off", "start", "len", "term"} of spans.reference over the compressed documents (lowered: over their lower-case
    forms), the rows the oracle's, the starts mapped back (a long document is ASCII: lowering moves nothing in it)"""
    import spans as S
    docs, maps = compressed(long_len)
    c = S.case("the long batch", EXPRS, lowered_docs(docs) if lowered else docs)
    total, so, st, ln, tm = S.reference(c)
    st = [_back(maps, d, st[k]) for d in range(len(docs)) for k in range(so[d], so[d + 1])]
    return {"span_off": so, "start": st, "len": ln, "term": tm, "rows": c.rows}


@functools.lru_cache(maxsize=None)
def sparse_mapped(long_len=None):
    """{"start", "len"}: the spans of sparse_hit_spans(True) -- of the lowered batch -- as spans of the batch itself, by
    lowermap_cases.expected over the compressed documents"""
    import lowermap_cases as LM
    import spans as S
    docs, maps = compressed(long_len)
    low = lowered_docs(docs)
    c = S.case("the long batch", EXPRS, low)
    total, so, st, ln, tm = S.reference(c)
    per = [(np.asarray(st[so[d]:so[d + 1]], np.int64), np.asarray(ln[so[d]:so[d + 1]], np.int64)) for d in range(len(docs))]
    w = LM.expected(docs, per)
    assert w is not None
    start = [_back(maps, d, int(w[1][k])) for d in range(len(docs)) for k in range(so[d], so[d + 1])]
    return {"start": start, "len": [int(v) for v in w[2]]}


@functools.lru_cache(maxsize=None)
def sparse_words(long_len=None):
    """the batch's spans (span_off, start, len) filtered at word borders -> {"out_off", "pos", "len", "kept"}: word_cases.kept on the
    island documents, and on the sixteen bytes round a span of a long document"""
    import word_cases as W
    lb = long_batch(long_len)
    out_off, pos, ln, kept = [0], [], [], []
    for d, doc in enumerate(lb.docs):
        for a, n, _ in doc.spans:
            if doc.body is not None:
                k = W.kept(doc.body, a, a + n)
            else:
                s, e = max(0, a - 8), min(doc.length, a + n + 8)
                k = W.kept(lb.read(lb.off[d] + s, lb.off[d] + e).tobytes(), a - s, a + n - s)
            kept.append((d, k))
            if k:
                pos.append(a)
                ln.append(n)
        out_off.append(len(pos))
    return {"out_off": out_off, "pos": pos, "len": ln, "kept": kept}


SPARSE = {"mark": sparse_mark, "replace": sparse_replace, "redact": sparse_redact, "excerpt": sparse_excerpt, "lower": sparse_lower,
          "route": sparse_route}
GROWING = ("mark", "replace", "lower")


@functools.lru_cache(maxsize=None)
def sparse(call, long_len=None):
    return SPARSE[call](long_batch(long_len))


def materialise(segs, text):
    """the output blob of a segment list over the batch's bytes (the scaled-down twin only)"""
    return b"".join(text[s[1]:s[2]] if s[0] == "text" else s[1] for s in segs)


def dense_reference(call, lb):
    """the module's own reference over the whole scaled-down batch, as one case -> the same dict as sparse(call), "out" for "segs" """
    import excerpts as X
    import mark as M
    import replace as R
    import route_docs as RD
    import tolower_cases as TC
    docs = lb.bodies()
    spans = [d.spans for d in lb.docs]
    two = [[s[:2] for s in sp] for sp in spans]
    if call == "mark":
        return M.expected(M.Case("twin", docs, two, OPEN, CLOSE))
    if call == "replace":
        return R.expected(R.Case("twin", docs, spans, REPS, KEY_REP))
    if call == "excerpt":
        return X.expected(X.Case("twin", docs, two, BEFORE, AFTER, True))
    if call == "redact":
        out = bytearray(lb.dense())
        for d, sp in enumerate(two):
            for a, n in sp:
                out[lb.off[d] + a:lb.off[d] + a + n] = bytes([MASK]) * n
        return {"out": bytes(out), "total": lb.total}
    if call == "lower":
        out, off = TC.reference(docs)
        return {"out": out, "total": len(out), "out_off": [int(v) for v in off]}
    assert call == "route"
    rows, masks = route_rows(lb)
    data, off, idx, bd, bb = RD.reference(lb.dense(), lb.off, rows, N_COLS, masks, ROUTE_MODE, ROUTE_REST, None)
    return {"out": data, "total": len(data), "out_off": off, "doc_idx": idx, "bucket_doc": bd, "bucket_byte": bb}


# ---- the comparison both tests use ----------------------------------------------------------------------------------------------------
def compare(want, got, seg_same):
    """None, or what differs first.  want: a sparse reference; got: {name: list or int} of the call's array outputs and totals;
    seg_same(out_lo, segment) -> bool: do the output's bytes from out_lo on equal the segment?  The arrays exactly; the blob
    segment by segment, the segments tiling [0, total)"""
    for k, w in want.items():
        if k == "segs":
            continue
        g = got[k]
        if isinstance(w, int):
            if int(g) != w:
                return "%s: got %d, want %d" % (k, int(g), w)
            continue
        g = [int(v) for v in g]
        if len(g) != len(w):
            return "%s: %d entries, want %d" % (k, len(g), len(w))
        if g != w:
            i = next(i for i in range(len(w)) if g[i] != w[i])
            return "%s[%d]: got %d, want %d" % (k, i, g[i], w[i])
    at = 0
    for s in want["segs"]:
        n = seg_len(s)
        assert n > 0
        if not seg_same(at, s):
            return "the output's bytes [%d, %d) differ from %s" % (at, at + n, s if s[0] == "text" else ("bytes", "%d of them" % n))
        at += n
    if at != want["total"]:
        return "the segments cover %d bytes of %d" % (at, want["total"])
    return None


def crossings(call, lb=None):
    """(the input's position B, the output position of the byte at input position B, the net length change in front of island 4):
    both crossings of 2^32 lie inside island 4 when the change stays under 2 KiB"""
    lb = lb or long_batch()
    w = sparse(call) if lb is long_batch() else SPARSE[call](lb)
    d4 = lb.island_at[4]
    delta = w["out_off"][d4] - lb.off[d4]
    return lb.cross, w["out_off"][d4], delta


# ---- the mutants -----------------------------------------------------------------------------------------------------------------------
class Virtual:
    """the output a (possibly wrong) segment list describes, read lazily: seg_same for compare() evaluates the first KiB of every
    segment against it with the numpy filler.  placed: [(out_lo, segment)]; bytes no segment covers hold POISON"""

    def __init__(self, lb, placed):
        self.lb, self.placed = lb, sorted(placed, key=lambda p: p[0])
        self.los = [p[0] for p in self.placed]

    def read(self, lo, hi):
        out = np.full(hi - lo, POISON, np.uint8)
        i = max(bisect.bisect_right(self.los, lo) - 1, 0)
        while i < len(self.placed) and self.placed[i][0] < hi:
            at, s = self.placed[i]
            a, b = max(lo, at), min(hi, at + seg_len(s))
            if b > a:
                out[a - lo:b - lo] = self.lb.read(s[1] + a - at, s[1] + b - at) if s[0] == "text" else np.frombuffer(s[1], np.uint8)[a - at:b - at]
            i += 1
        return out

    def seg_same(self, at, s):
        n = min(seg_len(s), 1024)
        want = self.lb.read(s[1], s[1] + n) if s[0] == "text" else np.frombuffer(s[1], np.uint8)[:n]
        return np.array_equal(self.read(at, at + n), want)


def placed_of(segs):
    out, at = [], 0
    for s in segs:
        out.append((at, s))
        at += seg_len(s)
    return out


def _arrays(w):
    return {k: v for k, v in w.items() if k != "segs"}


def mutants(call, lb):
    """{name: (got arrays, Virtual output)} -- wrong answers of the kinds a 32-bit slip gives, each of which compare() must notice.
    A mutant that the call's outputs cannot express (no array past 2^32, say) is left out"""
    w = SPARSE[call](lb) if lb is not long_batch() else sparse(call)
    placed = placed_of(w["segs"])
    out = {}
    far = [i for i, (at, s) in enumerate(placed) if s[0] == "text" and s[1] >= B]
    if far:                                                         # a segment's source lowered by 2^32
        i = far[0]
        p = list(placed)
        p[i] = (p[i][0], ("text", p[i][1][1] - B, p[i][1][2] - B))
        out["source lowered by 2^32"] = (_arrays(w), Virtual(lb, p))
        # an absolute position doc_off[d] + start truncated to 32 bits before the add: the last far segment read from there
        i = far[-1]
        p = list(placed)
        p[i] = (p[i][0], ("text", p[i][1][1] & (B - 1), (p[i][1][1] & (B - 1)) + seg_len(p[i][1])))
        out["doc_off + start truncated"] = (_arrays(w), Virtual(lb, p))
    for k in ("out_off", "exc_off", "bucket_byte"):                 # an offset entry taken mod 2^32
        if k in w and any(v >= B for v in w[k]):
            a = _arrays(w)
            a[k] = [v & (B - 1) for v in w[k]]
            out["%s mod 2^32" % k] = (a, Virtual(lb, placed))
    # `at` / `delta` from a 32-bit prefix sum: what belongs past output position 2^32 lands 2^32 lower, over what lies there
    if w["total"] > B:
        p = [(at, s) for at, s in placed if at < B]
        p += [(at - B, s) for at, s in placed if at >= B]
        out["destinations from a 32-bit prefix sum"] = (_arrays(w), Virtual(lb, p))
    # a copy from the neighbouring long document at the same in-document position
    for i, (at, s) in enumerate(placed):
        if s[0] != "text" or seg_len(s) < 1024:
            continue
        d = bisect.bisect_right(lb.off, s[1]) - 1
        if d in lb.long_at and d != lb.long_at[0]:
            other = lb.long_at[lb.long_at.index(d) - 1]
            rel = s[1] - lb.off[d]
            if rel + 1024 <= lb.docs[other].length:
                p = list(placed)
                p[i] = (at, ("text", lb.off[other] + rel, lb.off[other] + rel + seg_len(s)))
                out["the neighbouring long document"] = (_arrays(w), Virtual(lb, p))
                break
    return out


REQUIRED_MUTANTS = ("source lowered by 2^32", "doc_off + start truncated", "destinations from a 32-bit prefix sum", "the neighbouring long document")


def assert_not_vacuous():
    """on the real layout (nothing of it materialised): the reference passes its own comparison, and every mutant is noticed by it;
    every call has the mutants its outputs can express, and over the calls each kind of the list occurs.  -> {call: [mutants]}"""
    lb = long_batch()
    told = {}
    for call in SPARSE:
        w = sparse(call)
        ok = Virtual(lb, placed_of(w["segs"]))
        d = compare(w, _arrays(w), ok.seg_same)
        assert d is None, "%s: the reference fails its own comparison: %s" % (call, d)
        ms = mutants(call, lb)
        for name, (arrays, virt) in ms.items():
            assert compare(w, arrays, virt.seg_same) is not None, "%s: the mutant %r passes the comparison" % (call, name)
        told[call] = sorted(ms)
        # (the excerpts are a few KiB: their output has no position past 2^32 and no segment of a KiB; what they can get wrong is
        # where they read)
        required = REQUIRED_MUTANTS[:2] if call == "excerpt" else REQUIRED_MUTANTS
        missing = [m for m in required if m not in ms]
        assert not missing, (call, missing)
    assert "bucket_byte mod 2^32" in told["route"] and all("out_off mod 2^32" in told[c] for c in ("mark", "replace", "lower", "route"))
    return told
