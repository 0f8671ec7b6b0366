"""Text that lies anywhere (test infrastructure: numpy only, no GPU, nothing of the product loaded at import): two dictionaries
with every length class of the scan kernels' verification code, document lists whose borders -- between documents, in front of
the first and behind the last -- cut keywords at every split, `place`, which puts such a list at any residue of the 16-byte grid
behind any number of lead bytes, and the surroundings that fill the lead bytes and the 64 bytes of slack with what a scan must
not read as text: the missing half of the cut keyword, lead and continuation bytes of a rune, the batch's own text (what a bucket
run inside a routed blob sees).  Expectations are computed once on the bare documents with doc_off[0] == 0 and never know of a
placement.  Shared by test_placement_host.py (the lists are what they claim) and test_gpu_placement.py (the kernels).

The dictionaries hold lower-case keywords, as the DSL parser hands them to gft_build; the mixed-case spellings for fold=True are
in the documents.  No tests in here."""
import collections
import functools

import numpy as np

from long_terms import brute_force
from oracle.pyoracle import POS_END, POS_START, Oracle, pack_strings

POS_MODES = (POS_START, POS_END)
FILL = 0xEE                                     # in front of the text pointer and behind the slack
SLACK = 64
KINDS = ("zeros", "ones", "completes", "rune", "neighbour")
# (at, lead_len): every residue at % 16 of {0, 1, 3, 8, 15}, every lead length of {0, 1, 3, 4, 6, 7, 22, 23, 24, 40} -- both sides
# of the kernels' thresholds doc_abs + p >= 4, doc_abs < 7 and doc_abs < 23
PLACEMENTS = ((0, 0), (1, 0), (3, 1), (8, 3), (15, 4), (1, 6), (0, 7), (3, 22), (15, 23), (8, 24), (15, 40), (1, 23))
LEADS = tuple(sorted({l for _, l in PLACEMENTS}))

_ALPHA = b"abcdefghijklmnopqrstuvwxyz  ,.0123456789"


def _rng(*salt):
    return np.random.default_rng([20261019, *salt])


def _noise(rng, n, upper=0.1):
    """n bytes of filler; a tenth of the letters in upper case"""
    a = np.frombuffer(_ALPHA, np.uint8)[rng.integers(0, len(_ALPHA), n)].copy()
    up = (rng.random(n) < upper) & (a >= 97) & (a <= 122)
    a[up] -= 32
    return a.tobytes()


def _word(rng, n):
    """a keyword of n lower-case letters that the filler will not spell by chance"""
    return bytes(b"bdfghjklmpvw"[int(i)] for i in rng.integers(0, 12, n))


# ---- the dictionaries ----------------------------------------------------------------------------------------------------
T10 = b"placement7"                              # the 10-byte keyword; the text of every list begins with T10[4:]
T24 = b"sixteen byte grid lines."
T26 = b"bytes in front of doc zero"
T33 = b"every residue of the 16" + T10           # ends with T10: one lead completes both
T300 = _noise(_rng(300), 267, upper=0) + T33     # ... and, had it room, this one (the term_blob compare)
E10 = b"nationwide"                              # "nation" + 4: the text of every list ends with E10[:8]
E33 = E10 + b" slack behind the blobs"           # begins with E10: one tail completes both
WRAP = E10[5:8] + T10[4:]                        # the end of the text followed by its beginning ("neighbour")
HEAD, BEGIN = T300[:-6], T10[4:]                 # in front of the text / the text's first bytes
END, REST = E10[:8], E33[8:]                     # the text's last bytes / behind the text
assert (len(T24), len(T26), len(T33), len(T300), len(E33)) == (24, 26, 33, 300, 33)

SHARED_SUFFIX = [b"station", b"nation", b"ration", b"motion", b"lotion", b"notion", b"potion", b"caution", b"portion", b"section",
                 b"fraction", b"traction"]      # one anchor window for twelve keywords: the table compiler shifts some anchors
ONE_PLUS = [b"nations", b"national", b"nationals", E10, b"stationer", b"motions"]       # another keyword plus 1 to 4 bytes


def _dictionary():
    rng = _rng(1)
    t = [b"q", b"7", b"zx", b"q7", b"kjq", b"zxq", b"7.7",                               # 1, 2, 3 bytes: short-term records
         b"wxyz", b"grid", b"tion",                                                      # exactly 4: the window alone
         b"alpha", b"offset", b"residue", b"boundary", WRAP, T10, b"lead bytes", b"doc off zero", b"sixteen-byte grid",
         _word(rng, 23), T24,                                                            # 5 to 24: the slot's inline front
         _word(rng, 25), T26, _word(rng, 27), _word(rng, 28),                            # 25 to 28
         _word(rng, 29), _word(rng, 32), T33, E33, _word(rng, 40),                       # 29 to 40
         T300]
    t += SHARED_SUFFIX + ONE_PLUS
    t += [_word(rng, n) for n in (5, 6, 7, 9, 11, 13, 15, 17, 19, 21, 22, 24, 26, 31, 36)]
    assert len(set(t)) == len(t) and 60 <= len(t) <= 80
    return t


TERMS_ASCII = _dictionary()
CAFE, DEGREES = "café au lait".encode(), "30°c".encode()
MIXED_WRAP = DEGREES[1:3] + CAFE[4:7]            # "0" C2 + A9 " a": the mixed text's end followed by its beginning
TERMS_MIXED = TERMS_ASCII + [s.encode() for s in ("é", "É", "ß", "€", "café", "straße", "École", "10€", "naïve")] + [CAFE, DEGREES, MIXED_WRAP]
assert len(TERMS_MIXED) <= 80
# one representative keyword per length class; every split of each is an interior border
REPRESENTATIVES = [b"zx", b"kjq", b"wxyz", T10, T24, T26, T33, T300, E10]


def length_classes(terms):
    """how many keywords each class of the verification code gets"""
    c = collections.Counter()
    for t in terms:
        n = len(t)
        c["1-3" if n < 4 else "4" if n == 4 else "5-24" if n <= 24 else "25-28" if n <= 28 else "29-40" if n <= 40 else "long"] += 1
    return c


# ---- the documents ---------------------------------------------------------------------------------------------------------
def _splits(t):
    return range(1, len(t)) if len(t) <= 40 else (1, 3, 4, len(t) // 2, len(t) - 4, len(t) - 1)


def _dense(rng, terms, n):
    """about n bytes of keywords back to back, some of them spelt in mixed case"""
    out = []
    while sum(map(len, out)) < n:
        t = terms[int(rng.integers(0, len(terms)))]
        if len(t) > 40:
            continue
        if rng.random() < 0.3:
            t = bytes(b - 32 if 97 <= b <= 122 and rng.random() < 0.5 else b for b in t)
        out.append(t + (b" " if rng.random() < 0.5 else b""))
    return b"".join(out)


@functools.lru_cache(maxsize=None)
def _short():
    """-> (documents, planted): planted = the d for which the border between documents d and d + 1 cuts a keyword"""
    rng = _rng(2)
    docs, planted = [b"", BEGIN + _noise(rng, 90)], []
    docs += [b"q", T10, b"x", T300, b"7", _dense(rng, TERMS_ASCII, 300), T10.upper() + b" " + E10.title() + b" Q7 ZXQ " + T24.upper()]
    for t in REPRESENTATIVES:
        for k in _splits(t):
            planted.append(len(docs))
            a, b = (min(int(i), 390 - len(t)) for i in rng.integers(20, 200, 2))
            docs += [_noise(rng, a) + t[:k], t[k:] + _noise(rng, b)]
        if t == T10:
            docs += [b"", b"", b""]
    docs += [_dense(rng, TERMS_ASCII, 350), _noise(rng, 90) + END, b""]
    assert all(len(d) <= 400 for d in docs)
    return docs, planted


def _long_doc(rng):
    n = 2 * 8192 + 37
    a, b = _dense(rng, TERMS_ASCII, 64), _dense(rng, TERMS_ASCII, 64)
    d = BEGIN + a + _noise(rng, n // 2) + _dense(rng, TERMS_ASCII, 200) + T300
    return d + _noise(rng, n - len(d) - len(b) - len(END)) + b + END


@functools.lru_cache(maxsize=None)
def _long():
    rng = _rng(3)
    docs, planted = _short()
    first, last = _long_doc(rng), _long_doc(rng)
    assert len(first) == len(last) == 2 * 8192 + 37
    # (the first long document ends with END and the text behind it begins with BEGIN: WRAP lies across that border, and across
    # the one in front of the last long document)
    return [first] + docs + [last], [0] + [d + 1 for d in planted] + [len(docs) - 1]


def _mixed(core):
    """a list for TERMS_MIXED: its first byte is a continuation byte that a C3 in front would make a letter, its last byte a lead
    byte that a continuation byte behind it would complete; in between, runes whole and cut by document borders"""
    docs, planted = core
    rng = _rng(4)
    front = [b"", CAFE[4:] + b" " + _noise(rng, 40)]
    inner = docs[1:-1] if docs[0] == b"" else docs           # (the short list: its empty first and last documents are these lists' own)
    shift = len(front) - (1 if docs[0] == b"" else 0)
    latin = ["vive la école, café crème".encode(), "STRAßE straße 10€ naïve".encode(), "École É é".encode(), "€".encode(), "ß".encode(),
             _noise(rng, 30) + "caf".encode() + b"\xc3", b"\xa9 " + _noise(rng, 30),                      # "café" cut inside its rune
             _noise(rng, 30) + "10".encode() + b"\xe2\x82", b"\xac" + _noise(rng, 30),                    # "10€" cut inside its rune
             "é".encode() * 40, _noise(rng, 60) + "ß".encode() + _noise(rng, 60)]
    n0 = len(front) + len(inner)
    return front + inner + latin + [_noise(rng, 50) + DEGREES[:3], b""], [d + shift for d in planted] + [n0 + 5, n0 + 7]


def fold_safe(doc):
    """k_fold_safe's rule for ONE document (include/gft.h, gft_last_nonascii): ASCII, C2 80..BF, C3 9F..BF and C3 97"""
    i = 0
    while i < len(doc):
        b = doc[i]
        if b < 0x80:
            i += 1
            continue
        if b not in (0xC2, 0xC3) or i + 1 >= len(doc) or not 0x80 <= doc[i + 1] <= 0xBF:
            return False
        if b == 0xC3 and not (doc[i + 1] >= 0x9F or doc[i + 1] == 0x97):
            return False
        i += 2
    return True


Batch = collections.namedtuple("Batch", "name terms docs planted head begin end rest")


@functools.lru_cache(maxsize=None)
def batch(name):
    """"short" / "long" (TERMS_ASCII), "short_mixed" / "long_mixed" (TERMS_MIXED), "<x>_mixed_safe": the fold-safe documents of a
    mixed list (its borders are no longer the planted ones), "short_lines": DOCS_SHORT with a newline behind every document.
    head / rest: what would complete, in front of the text and behind it, the keyword that the text's first bytes (begin) lack and
    the one that its last bytes (end) start"""
    if name in ("short", "long"):
        docs, planted = _short() if name == "short" else _long()
        return Batch(name, TERMS_ASCII, docs, tuple(planted), HEAD, BEGIN, END, REST)
    if name in ("short_mixed", "long_mixed"):
        docs, planted = _mixed(_short() if name == "short_mixed" else _long())
        return Batch(name, TERMS_MIXED, docs, tuple(planted), b"caf\xc3", CAFE[4:], DEGREES[:3], DEGREES[3:] + b" ")
    if name == "short_lines":                                # DOCS_SHORT as the lines of a blob: one newline behind every document
        docs = [d.replace(b"\n", b" ") + b"\n" for d in _short()[0]]
        return Batch(name, TERMS_ASCII, docs, (), b"", b"", b"", b"")
    base = batch(name[:-len("_safe")])
    docs = [d for d in base.docs if fold_safe(d)]
    return Batch(name, TERMS_MIXED, docs, (), HEAD, BEGIN, b"", b"")


DOCS_SHORT, DOCS_LONG = batch("short").docs, batch("long").docs
DOCS_SHORT_MIXED, DOCS_LONG_MIXED = batch("short_mixed").docs, batch("long_mixed").docs
BATCHES = ("short", "long", "short_mixed", "long_mixed", "short_mixed_safe", "long_mixed_safe")


# ---- where the text lies ---------------------------------------------------------------------------------------------------
def place(docs, lead, tail, at):
    """-> (buffer uint8, doc_off uint64 [n + 1], text_start): `at` bytes of 0xEE, lead, the documents, tail padded with 0xEE to 64
    bytes at least, 16 bytes more.  The text pointer is buffer + text_start (= at) and doc_off[0] == len(lead)"""
    text = b"".join(docs)
    tail = bytes(tail) + bytes([FILL]) * max(0, SLACK - len(tail))
    buf = bytes([FILL]) * at + bytes(lead) + text + tail + bytes([FILL]) * 16
    off = np.zeros(len(docs) + 1, dtype=np.uint64)
    off[0] = len(lead)
    if docs:
        off[1:] = len(lead) + np.cumsum([len(d) for d in docs], dtype=np.uint64)
    return np.frombuffer(buf, dtype=np.uint8).copy(), off, at


def surroundings(kind, lead_len, b):
    """-> (lead, tail) of `kind` for batch b; a lead longer than what the kind has to say is padded in front"""
    text = b"".join(b.docs)
    if kind == "zeros":
        return bytes(lead_len), bytes(SLACK)
    if kind == "ones":
        return b"\xff" * lead_len, b"\xff" * SLACK
    if kind == "completes":
        return (b"~" * lead_len + b.head)[len(b.head):], b.rest       # (the last lead_len bytes)
    if kind == "rune":
        return b"\xc3" * lead_len, b"\x89" * SLACK            # (tolower_cases.pack: a lead byte in front, a continuation byte behind)
    if kind == "neighbour":
        own = text * (lead_len // max(len(text), 1) + 1) if text else bytes(lead_len)
        return own[len(own) - lead_len:], (text + bytes(SLACK))[:SLACK]
    raise ValueError(kind)


def placed(name, kind, at, lead_len):
    b = batch(name)
    lead, tail = surroundings(kind, lead_len, b)
    assert len(lead) == lead_len
    return place(b.docs, lead, tail, at)


# ---- expectations: the bare documents, doc_off[0] == 0 ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def expected_csr(name, pos_mode, fold):
    """(match_off, term_id, pos) by long_terms.brute_force; read-only"""
    b = batch(name)
    got = brute_force(b.terms, b.docs, pos_mode, fold)
    for a in got:
        a.setflags(write=False)
    return got


def _q(t):
    return '"%s"' % t.decode("utf-8")


PRESENCE, POSITIONS = "presence", "positions"


@functools.lru_cache(maxsize=None)
def expressions(which):
    """PRESENCE: one UNIT per keyword of TERMS_ASCII and a dozen AND / OR / NOT expressions -- no position is read;
    POSITIONS: the same plus six INORD groups over the keywords that the borders cut"""
    t = sorted(TERMS_ASCII)
    e = [_q(x) for x in t]
    e += ['%s and %s' % (_q(T10), _q(E10)), '%s or %s' % (_q(WRAP), _q(T33)), 'not %s' % _q(T10), '%s and not (%s or %s)' % (_q(b"q"), _q(WRAP), _q(E33)),
          '%s and not %s' % (_q(b"q"), _q(b"zx")), '(%s or %s) and %s' % (_q(T24), _q(T26), _q(b"tion")), 'not (%s or %s)' % (_q(T300), _q(E10)),
          '%s and %s and %s' % (_q(b"nation"), _q(b"nations"), _q(b"national")), '%s or %s or %s' % (_q(b"kjq"), _q(b"wxyz"), _q(b"7.7")),
          'not %s or %s' % (_q(b"grid"), _q(T24)), '%s and not (%s and %s)' % (_q(b"q7"), _q(b"zxq"), _q(b"alpha")),
          '%s and %s' % (_q(T300), _q(T33))]
    if which == POSITIONS:
        e += ['inord(%s and %s)' % (_q(T10), _q(E10)), 'inord(%s and %s)' % (_q(E10), _q(T10)), 'inord(%s and %s and %s)' % (_q(b"q"), _q(b"zx"), _q(b"kjq")),
              'inord((%s or %s) and %s)' % (_q(WRAP), _q(T33), _q(b"tion")), 'inord(%s and (%s or %s))' % (_q(b"nation"), _q(T24), _q(T26)),
              'not (inord(%s and %s))' % (_q(b"wxyz"), _q(T10))]
    return tuple(e)


@functools.lru_cache(maxsize=None)
def expected_rows(name, which, fold):
    """the bitmap of Oracle.process over the bare documents; read-only"""
    b = batch(name)
    o = Oracle(b.terms)
    o.set_expressions(list(expressions(which)), True)
    blob, off = pack_strings(b.docs)
    rows = o.process(blob, off, fold=fold)
    rows.setflags(write=False)
    return rows


# ---- the lists are what they claim ------------------------------------------------------------------------------------------------
def straddlers(name, kind, lead_len):
    """brute force over the whole placed text -- lead, documents and slack as ONE document -- -> {border: matches across it} for
    the borders doc_off[0] ("first"), doc_off[n] ("last") and the planted interior ones (their document index), and the matches
    that lie inside one document, as a CSR like expected_csr's"""
    b = batch(name)
    buf, off, at = placed(name, kind, 0, lead_len)
    whole = bytes(buf[:int(off[-1]) + SLACK])
    _, tid, pos = brute_force(b.terms, [whole], POS_START, False)
    dictionary = sorted(set(b.terms))
    start = pos.astype(np.int64)
    end = start + np.asarray([len(dictionary[i]) for i in tid], dtype=np.int64)           # one past the last byte
    across = {}
    for key, at in [("first", int(off[0])), ("last", int(off[-1]))] + [(d, int(off[d + 1])) for d in b.planted]:
        across[key] = int(np.count_nonzero((start < at) & (end > at)))
    # matches wholly inside a document: what a scan of the placed text has to answer
    d_of = np.searchsorted(off, start, side="right") - 1
    inside = (start >= int(off[0])) & (end <= int(off[-1]))
    inside &= end <= off[np.clip(d_of + 1, 0, len(off) - 1)].astype(np.int64)
    return across, int(np.count_nonzero(inside))


def assert_not_vacuous():
    """conditions, not measurements: the surroundings really hold what a scan must not take for text"""
    for t in (TERMS_ASCII, TERMS_MIXED):
        c = length_classes(t)
        assert all(c[k] for k in ("1-3", "4", "5-24", "25-28", "29-40", "long")), c
    for name in ("short", "long", "short_mixed", "long_mixed"):
        b = batch(name)
        text = b"".join(b.docs)
        assert text.startswith(b.begin) and text.endswith(b.end)
        assert name == "long" or (b.docs[0] == b"" and b.docs[-1] == b"")
        assert b.planted and all(0 <= d < len(b.docs) - 1 for d in b.planted)
        total = int(expected_csr(name, POS_START, False)[0][-1])
        for kind in ("completes", "neighbour"):
            for lead_len in (l for l in LEADS if l >= 7):
                across, inside = straddlers(name, kind, lead_len)
                assert across["first"] >= 1, (name, kind, lead_len, "nothing lies across doc_off[0]")
                assert across["last"] >= 1, (name, kind, lead_len, "nothing lies across doc_off[n]")
                missing = [d for d in b.planted if across[d] < 1]
                assert not missing, (name, kind, lead_len, "no match across the borders behind documents", missing)
                # none of them is in the expectation: it holds the matches inside one document and nothing else
                assert inside == total, (name, kind, lead_len, inside, total)
    for name in ("short_mixed", "long_mixed"):
        text = b"".join(batch(name).docs)
        lead, tail = surroundings("rune", 7, batch(name))
        assert fold_safe(lead[-1:] + text[:1]) and not fold_safe(text[:1])         # across the border a letter, alone a stray byte
        assert fold_safe(text[-1:] + tail[:1]) and not fold_safe(text[-1:])
    for name in ("short_mixed_safe", "long_mixed_safe"):
        docs = batch(name).docs
        assert len(docs) > 200 and any(max(d, default=0) >= 0x80 for d in docs)
    assert all(len(d) <= 400 for d in DOCS_SHORT) and 200 <= len(DOCS_SHORT) <= 300
    assert len(DOCS_LONG[0]) == len(DOCS_LONG[-1]) == 2 * 8192 + 37
    assert {a % 16 for a, _ in PLACEMENTS} == {0, 1, 3, 8, 15} and set(LEADS) == {0, 1, 3, 4, 6, 7, 22, 23, 24, 40} and (0, 0) in PLACEMENTS
