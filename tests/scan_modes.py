"""The two answer modes behind the scan (test infrastructure: numpy only, no GPU, nothing of the product loaded at import):
GFT_POS_RUNES (k_rune_doc_blocks, k_rune_block_starts, k_pos_to_rune) and GFT_SCAN_UNIQUE (k_unique_terms), with cases built from
the kernels' own borders -- counted blocks of 64 bytes, documents, the exclusive scan's tile of 4096, rounds of 256 matches, waves
of 64, a first-occurrence row per workgroup -- and references that share no code with the kernels or with oracle/runes_ref.py.

Rune reference: Go's decoder restated with Python's STRICT decoder (the rune at b[i] is n bytes wide if b[i:i+n] decodes to one
character, else 1); t[p] = rune starts in [0, p), and a position inside a rune counts that rune as started.  The rune dictionary
holds every byte that the texts use as a keyword of its own, so every byte position of every document is a match and the whole
table is compared; a few multi-byte keywords put ties at one position into the canonical CSR.
Unique reference: dict.fromkeys over the full match list (the oracle's; for the small cases also bytes.find).

Shared by test_scan_modes_host.py (the references and the cases are what they claim) and test_gpu_scan_modes.py (the kernels).
No tests in here."""
import collections
import functools
import itertools

import numpy as np

from long_terms import brute_force
from oracle.pyoracle import POS_START, Oracle, pack_strings

RUNE_BLOCK = 64                                  # kRuneBlock
SCAN_TILE = 4096                                 # kScanTile: the exclusive scan over documents and over counted blocks
ROUND, WAVE = 256, 64                            # k_unique_terms: matches per round, lanes per wave
# unique_pipeline's grid is min(n_docs, 4 * CUs) workgroups (fewer only past 256 MB of rows); workgroup w visits the documents
# w, w + grid, w + 2 grid, ... with ONE first-occurrence row.  4 * CUs for the CU counts of the CDNA parts:
GRIDS = tuple(4 * cu for cu in (64, 104, 110, 120, 128, 208, 220, 228, 256, 304))
ROW_REUSE_DOCS = 5000                            # > 4 * 304 many times over

# the 24 bytes of the sweep: ASCII, every edge of the continuation ranges, every class of lead byte
ALPHABET = bytes.fromhex("417F808F909FA0BFC0C1C2DFE0E1ECEDEEEFF0F1F3F4F5FF")
assert len(set(ALPHABET)) == 24


def _rng(*salt):
    return np.random.default_rng([20261020, *salt])


# ---- the rune reference ------------------------------------------------------------------------------------------------------
def rune_width(b, i):
    """width of the rune that Go's decoder reads at b[i]: Python's strict decoder accepts b[i:i+n] as ONE character, or 1"""
    if b[i] < 0x80:
        return 1
    for n in (2, 3, 4):
        s = b[i:i + n]
        if len(s) == n:
            try:
                if len(s.decode("utf-8")) == 1:
                    return n
            except UnicodeDecodeError:
                pass
    return 1


def rune_table(b, width=rune_width):
    """t[p] = number of rune starts in [0, p), p in 0 .. len(b)"""
    b = bytes(b)
    start = np.zeros(len(b) + 1, dtype=np.int64)
    i = 0
    while i < len(b):
        start[i + 1] = 1
        i += width(b, i)
    return np.cumsum(start)


# ---- wrong readings of the rune contract (assert_not_vacuous) ---------------------------------------------------------------------
def _replace_width(b, i):
    """errors="replace" groups a maximal invalid prefix into ONE replacement character (Go emits one per byte)"""
    w = rune_width(b, i)
    if w > 1 or b[i] < 0x80:
        return w
    try:
        b[i:i + 4].decode("utf-8")
    except UnicodeDecodeError as e:
        if e.start == 0:
            return max(1, e.end - e.start)
    return 1


def table_replace(doc):
    return rune_table(doc, _replace_width)


def table_blocks(doc):
    """every counted block decoded as a document of its own: no look-back over its first byte, no look-ahead past its last"""
    out, base = [np.zeros(1, np.int64)], 0
    for a in range(0, len(doc), RUNE_BLOCK):
        t = rune_table(doc[a:a + RUNE_BLOCK])
        out.append(base + t[1:])
        base += int(t[-1])
    return np.concatenate(out)


def table_bytes(doc):
    return np.arange(len(doc) + 1, dtype=np.int64)


def tables_unbounded(lead, docs, tail):
    """a decoder that knows no document: one walk over lead + text + tail, counted from each document's first byte"""
    whole = rune_table(bytes(lead) + b"".join(docs) + bytes(tail))
    out, at = [], len(lead)
    for d in docs:
        # (a rune that began in front of the document swallows the document's first bytes: they start nothing)
        out.append(whole[at:at + len(d) + 1] - whole[at])
        at += len(d)
    return out


# ---- forms -----------------------------------------------------------------------------------------------------------------------
E_ACUTE, EURO, CLEF = "é".encode(), "€".encode(), "\U0001d11e".encode()         # C3 A9 / E2 82 AC / F0 9D 84 9E
FORMS = collections.OrderedDict([
    ("two", E_ACUTE), ("three", EURO), ("four", CLEF),
    ("two-1", E_ACUTE[:1]), ("three-1", EURO[:2]), ("three-2", EURO[:1]), ("four-1", CLEF[:3]), ("four-2", CLEF[:2]),
    ("overlong-c0", b"\xc0\x80"), ("overlong-c1", b"\xc1\xbf"), ("overlong-e0", b"\xe0\x80\x80"), ("overlong-f0", b"\xf0\x80\x80\x80"),
    ("surrogate", b"\xed\xa0\x80"), ("past-10ffff", b"\xf4\x90\x80\x80"), ("f5", b"\xf5"), ("ff", b"\xff"),
    ("lead-lead-2", b"\xc3\xc3\xa9"), ("lead-lead-3", b"\xe2\xe2\x82\xac"), ("lead-lead-4", b"\xf0\xe2\x82\xac"), ("lead-lead-34", b"\xe2\x82\xf0\x9d\x84\x9e"),
    ("stray-1", b"\x80"), ("stray-2", b"\xbf\x80"), ("stray-3", b"\x80\xbf\x80"), ("stray-4", b"\x80" * 4), ("stray-5", b"\x9f\x80\xa0\xbf\x80"),
    ("four+1", CLEF + b"\x80"), ("edge-e0", b"\xe0\xa0\x80"), ("edge-ed", b"\xed\x9f\xbf"), ("edge-f0", b"\xf0\x90\x80\x80"), ("edge-f4", b"\xf4\x8f\xbf\xbf"),
])
MARK_L, MARK_R = b"<", b">"
FILLER = b"abcdefghijklmnopqrstuvwxyz "
KEYWORDS = [E_ACUTE, EURO + b"uro", CLEF, b"<" + E_ACUTE, b"ab"]                 # ties at one position of the canonical CSR
NO_MATCH = b"#$%&\x81\xb0\xc4\xe5\xf2"                                           # bytes that no keyword holds


def _rune_dictionary():
    used = set(ALPHABET) | set(FILLER) | set(MARK_L + MARK_R) | set(b"AZQ") | {b for f in FORMS.values() for b in f} | {b for k in KEYWORDS for b in k}
    assert not used & set(NO_MATCH)
    return [bytes([b]) for b in sorted(used)] + KEYWORDS


RUNE_TERMS = _rune_dictionary()


def _fill(rng, n):
    return bytes(FILLER[int(i)] for i in rng.integers(0, len(FILLER), n))


# ---- cases -------------------------------------------------------------------------------------------------------------------------
# names[d] says what document d is for (a failing comparison is located by it); lead / tail: what the device-resident call finds in
# front of doc_off[0] and in the slack (None: the test's own fillings only)
Case = collections.namedtuple("Case", "name terms docs names fold lead tail")


def make_case(name, docs, names=None, terms=None, fold=False, lead=None, tail=None):
    names = list(names) if names is not None else ["%s[%d]" % (name, d) for d in range(len(docs))]
    assert len(names) == len(docs)
    return Case(name, RUNE_TERMS if terms is None else terms, [bytes(d) for d in docs], names, fold, lead, tail)


@functools.lru_cache(maxsize=None)
def block_borders():
    """each form at every shift across byte 64 and across byte 128 of its document: its byte k on the border for every k, and one
    position to either side; ASCII filler, a marker byte directly in front and behind"""
    rng = _rng(1)
    docs, names = [], []
    for border in (RUNE_BLOCK, 2 * RUNE_BLOCK):
        for fname, f in FORMS.items():
            for at in range(border - len(f) - 1, border + 2):            # the form's first byte lies at `at`
                docs.append(_fill(rng, at - 1) + MARK_L + f + MARK_R + _fill(rng, int(rng.integers(0, 70))))
                names.append("%s at %d (border %d)" % (fname, at, border))
    return make_case("block_borders", docs, names)


def cuts():
    """(form name, k): every interior point of every form of two bytes or more"""
    return [(n, k) for n, f in FORMS.items() for k in range(1, len(f))]


@functools.lru_cache(maxsize=None)
def document_borders():
    """each form cut at every interior point between document d and document d + 1"""
    rng = _rng(2)
    docs, names = [], []
    for fname, k in cuts():
        f = FORMS[fname]
        docs += [_fill(rng, int(rng.integers(0, 70))) + MARK_L + f[:k], f[k:] + MARK_R + _fill(rng, int(rng.integers(0, 70)))]
        names += ["%s cut at %d: front" % (fname, k), "%s cut at %d: back" % (fname, k)]
    return make_case("document_borders", docs, names)


@functools.lru_cache(maxsize=None)
def edge_cut(fname, k, gname, j):
    """form f cut between the lead bytes and doc_off[0], form g between the last document and the slack (gft_scan_device): the
    lead ends in f[:k], the text begins with f[k:]; the text ends in g[:j], the slack begins with g[j:]"""
    rng = _rng(3, len(fname), k, len(gname), j)
    f, g = FORMS[fname], FORMS[gname]
    docs = [f[k:] + MARK_R + _fill(rng, 20), b"", _fill(rng, 70) + E_ACUTE, _fill(rng, 61) + MARK_L + g[:j]]
    return make_case("edge_cut %s|%d %s|%d" % (fname, k, gname, j), docs, lead=_fill(rng, 5) + f[:k], tail=g[j:])


def edge_cuts():
    c = cuts()
    return [edge_cut(f, k, *c[(i * 7 + 3) % len(c)]) for i, (f, k) in enumerate(c)]


LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129)


@functools.lru_cache(maxsize=None)
def document_lengths():
    """documents of the lengths around one and two counted blocks, of runes whole and broken, each ending in every way"""
    rng = _rng(4)
    docs, names = [], []
    for n in LENGTHS:
        for tail in (b"", E_ACUTE, EURO, CLEF, EURO[:2], CLEF[:3], b"\x80\x80"):
            if len(tail) > n:
                continue
            body = b""
            while len(body) < n - len(tail):
                body += (E_ACUTE, EURO, CLEF, b"x", b"\x80", b"\xe2\x82", _fill(rng, 3))[int(rng.integers(0, 7))]
            docs.append(body[:n - len(tail)] + tail)
            names.append("length %d ending in %s" % (n, tail.hex() or "nothing"))
    assert {len(d) for d in docs} == set(LENGTHS)
    return make_case("document_lengths", docs, names)


@functools.lru_cache(maxsize=None)
def empty_and_matchless():
    """runs of empty documents in front, between and at the end; documents of bytes outside the dictionary between documents that
    match (match_off and blk_base repeat: the two binary searches)"""
    rng = _rng(5)
    text = [EURO * 30 + b"x", _fill(rng, 64) + CLEF, E_ACUTE * 33, b"\x80" * 65, CLEF[:3] + b"a", _fill(rng, 129) + EURO[:2]]
    quiet = [NO_MATCH, NO_MATCH * 15, NO_MATCH[:1], NO_MATCH[4:] * 30]
    docs = [b""] * 3 + [text[0]] + [b""] * 5 + [text[1], quiet[0], text[2]] + [b""] + [quiet[1], quiet[2]] + [text[3]] + [b""] * 2 + [quiet[3]]
    docs += [b"", text[4], quiet[0], b"", quiet[1], text[5]] + [b""] * 4
    return make_case("empty_and_matchless", docs)


_SHORT = [b"", b"a", E_ACUTE, EURO, CLEF, b"\x80", EURO[:2], b"x" + CLEF[:3], CLEF + b"\x80", NO_MATCH[:2], b"\xc3", b"<" + E_ACUTE + b">", b"ab"]


@functools.lru_cache(maxsize=None)
def tile_batch(n):
    """n short documents (the scan's tile over documents: 1, 2, 4095, 4096, 4097)"""
    rng = _rng(6)
    pick = rng.integers(0, len(_SHORT), n)
    return make_case("tile_batch %d" % n, [_SHORT[int(i)] for i in pick])


TILE_BATCHES = (1, 2, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1)


@functools.lru_cache(maxsize=None)
def long_document():
    """one document of more than 4096 counted blocks (a little over 256 KiB) of multi-byte runes, whole and broken: it crosses the
    tile of the block scan and the scan's work units; a short document on either side"""
    rng = _rng(7)
    pieces = [E_ACUTE, EURO, CLEF, b"x", b"\x80", EURO[:2], b"ab", b"<" + E_ACUTE, CLEF[:3], b" "]
    pick = rng.integers(0, len(pieces), 120_000)
    doc = b"".join(pieces[int(i)] for i in pick)
    doc = doc[:(SCAN_TILE + 37) * RUNE_BLOCK + 5]
    assert len(doc) > SCAN_TILE * RUNE_BLOCK + 2000
    return make_case("long_document", [E_ACUTE + b"a", doc, CLEF])


@functools.lru_cache(maxsize=None)
def folded():
    """fold=True: ASCII folding keeps lengths, so the positions stay those of the caller's text"""
    docs = [b"AB" + CLEF[:2] + b"QZ<" + E_ACUTE + EURO + b"URO Euro " + CLEF + b"AB" * 40 + EURO[:2] + b"Z", b"", b"A\x80Z" + CLEF + b"Q"]
    return make_case("folded", docs, fold=True)


@functools.lru_cache(maxsize=None)
def random_documents(n=2000, longest=300, salt=8):
    """seeded documents of 0 to `longest` bytes over the 24-byte alphabet"""
    rng = _rng(salt)
    a = np.frombuffer(ALPHABET, np.uint8)
    docs = [a[rng.integers(0, 24, int(k))].tobytes() for k in rng.integers(0, longest + 1, n)]
    return make_case("random %d x %d" % (n, longest), docs)


def small_rune_cases():
    """the fixed cases whose lists are short enough for bytes.find and for the wrong readings"""
    return [block_borders(), document_borders(), document_lengths(), empty_and_matchless(), folded()]


# ---- expectations ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle(terms_key, pos_mode):
    return Oracle(list(terms_key), pos_mode)


def full_csr(case, pos_mode=POS_START):
    """the oracle's full match list of the bare documents (doc_off[0] == 0)"""
    return _full_csr(case.name, tuple(case.terms), tuple(case.docs), case.fold, pos_mode)


@functools.lru_cache(maxsize=None)
def _full_csr(name, terms, docs, fold, pos_mode):
    blob, off = pack_strings(list(docs))
    got = _oracle(terms, pos_mode).scan(blob, off, fold=fold)
    for a in got:
        a.setflags(write=False)
    return got


def rune_csr(case, table=rune_table):
    """full_csr with every position read through its document's table; read-only"""
    return _rune_csr(case.name, tuple(case.terms), tuple(case.docs), case.fold, table)


def map_positions(csr, tables):
    mo, ti, po = csr
    out = po.copy()
    for d, t in enumerate(tables):
        a, b = int(mo[d]), int(mo[d + 1])
        if b > a:
            out[a:b] = np.asarray(t, dtype=np.int64)[po[a:b].astype(np.int64)]
    out.setflags(write=False)
    return mo, ti, out


@functools.lru_cache(maxsize=None)
def _rune_csr(name, terms, docs, fold, table):
    return map_positions(_full_csr(name, terms, docs, fold, POS_START), [table(d) for d in docs])


def unique_lists(csr, order=None):
    """per document, every term once in the order of its first occurrence (order=sorted: the wrong reading by term id)"""
    mo, ti, _ = csr
    out = []
    for d in range(len(mo) - 1):
        first = list(dict.fromkeys(ti[int(mo[d]):int(mo[d + 1])].tolist()))
        out.append(order(first) if order else first)
    return out


def lists_to_csr(lists):
    mo = np.zeros(len(lists) + 1, dtype=np.uint64)
    if lists:
        mo[1:] = np.cumsum([len(x) for x in lists], dtype=np.uint64)
    ti = np.asarray(list(itertools.chain.from_iterable(lists)), dtype=np.uint32)
    return mo, ti, np.zeros(ti.size, dtype=np.uint32)


def unique_csr(case, pos_mode=POS_START):
    return _unique_csr(case.name, tuple(case.terms), tuple(case.docs), case.fold, pos_mode)


@functools.lru_cache(maxsize=None)
def _unique_csr(name, terms, docs, fold, pos_mode):
    got = lists_to_csr(unique_lists(_full_csr(name, terms, docs, fold, pos_mode)))
    for a in got:
        a.setflags(write=False)
    return got


def lists_with_stale_rows(lists, grid):
    """the wrong reading: a workgroup's row is not reset, so a document loses every term that the document the same workgroup
    visited before it (d - grid) holds"""
    return [[t for t in x if d < grid or t not in set(lists[d - grid])] for d, x in enumerate(lists)]


def brute_csr(case, pos_mode=POS_START):
    return brute_force(case.terms, case.docs, pos_mode, case.fold)


def per_document_multisets(csr):
    mo, ti, po = csr
    return [collections.Counter(zip(ti[int(mo[d]):int(mo[d + 1])].tolist(), po[int(mo[d]):int(mo[d + 1])].tolist())) for d in range(len(mo) - 1)]


# ---- unique cases ------------------------------------------------------------------------------------------------------------------
# 676 keywords "#xy": '#' begins every keyword and occurs nowhere else, so a text of k keywords back to back holds exactly k matches,
# in the order written, and the sorted dictionary's ids are 26 x + y
UNIQUE_TERMS = [b"#" + bytes([x, y]) for x in range(97, 123) for y in range(97, 123)]
COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 3 * ROUND + 5)
FIRST_AT = (WAVE - 2, WAVE - 1, WAVE, WAVE + 1, ROUND - 2, ROUND - 1, ROUND, ROUND + 1, ROUND + 2)      # "match number n" read from zero and from one


def _text(ids):
    return b"".join(UNIQUE_TERMS[int(i)] for i in ids)


@functools.lru_cache(maxsize=None)
def unique_fixed():
    rng = _rng(20)
    docs, names = [], []
    pool = rng.permutation(676)[:40]
    for n in COUNTS:                                            # matches per document around the rounds of 256 and the waves of 64
        docs.append(_text(pool[rng.integers(0, 40, n)]))
        names.append("%d matches" % n)
    for n in FIRST_AT:                                          # a term whose first occurrence is match n, and which comes again
        ids = list(pool[rng.integers(0, 39, 600)])              # (pool[39] is kept out)
        ids[n] = pool[39]
        ids[n + 200] = ids[599] = pool[39]
        docs.append(_text(ids))
        names.append("first occurrence at match %d" % n)
    ids = list(pool[rng.integers(0, 38, 3 * ROUND)])            # a term in round 0 that recurs only in round 2; one that appears in round 2 only
    ids[5], ids[2 * ROUND + 17], ids[2 * ROUND + 200] = pool[38], pool[38], pool[39]
    docs.append(_text(ids))
    names.append("recurs only in a later round")
    docs.append(_text([pool[7]] * 600))
    names.append("one term 600 times")
    docs.append(_text(range(675, 75, -1)))
    names.append("600 distinct terms, ids descending")
    docs.append(_text(rng.permutation(676)[:600]))
    names.append("600 distinct terms, shuffled")
    docs.append(_text(list(range(300, 240, -1)) * 5 + list(range(60))))
    names.append("order against term ids, repeated")
    docs.append(_text(rng.integers(0, 676, 20_000)))            # 60 000 bytes: longer than a work unit, 79 rounds
    names.append("longer than a work unit")
    return make_case("unique_fixed", docs, names, terms=UNIQUE_TERMS)


@functools.lru_cache(maxsize=None)
def unique_rows(n=ROW_REUSE_DOCS):
    """more documents than the grid has workgroups: one to six terms each out of twelve (so documents d and d + k share terms for
    some d and use disjoint sets for others, at every k), every eleventh document empty"""
    rng = _rng(21)
    pool = rng.permutation(676)[:12]
    docs = [b"" if d % 11 == 10 else _text(pool[rng.integers(0, 12, int(rng.integers(1, 7)))]) for d in range(ROW_REUSE_DOCS)]
    return make_case("unique_rows %d" % n, docs[:n], terms=UNIQUE_TERMS)


UNIQUE_BATCHES = (SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, ROW_REUSE_DOCS)


# ---- the sequence on one engine ------------------------------------------------------------------------------------------------------
SEQUENCE = (("plain", 200), ("unique", 3000), ("plain", 5000), ("runes", 5000), ("unique", 3000), ("runes+unique", 5000), ("plain", 200),
            ("runes", 200), ("unique", 200), ("plain", 3000))


@functools.lru_cache(maxsize=None)
def sequence_batch(n):
    return random_documents(n, 40, 9)


# ---- over two devices ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def two_device_batch():
    """two halves of equal bytes around a run of empty documents: the byte cut of a handle over two devices lands at the head of
    the run (the first of equal offsets), beside a rune cut by the run's borders"""
    rng = _rng(22)
    front = [_fill(rng, 50) + EURO + _fill(rng, 100), b"", _fill(rng, 120) + MARK_L + CLEF[:2]]
    back = [CLEF[2:] + MARK_R + _fill(rng, 118), b"", E_ACUTE * 10 + _fill(rng, 135)]
    assert sum(map(len, front)) == sum(map(len, back))
    return make_case("two_devices", front + [b""] * 6 + back)


# ---- the inputs of test_gpu_parity.test_rune_offsets_are_the_anknown_engine_positions ------------------------------------------------
def parity_rune_texts():
    texts = ["héllo wörld €uro \U0001d11e x lo", "", "x",
             b"\x80x\xc3 lo \xe2\x82 x \xed\xa0\x80lo \xf5x \xc0\x80 x\xf0\x9f lo".decode("latin-1"),
             ("é" * 40 + "x") * 30, "\U0001d11e" * 100 + "lo"]
    return [t.encode("latin-1") if i == 3 else t.encode("utf-8") for i, t in enumerate(texts)]


# ---- the cases are what they claim ---------------------------------------------------------------------------------------------------
def differing(case, want, got):
    """names of the documents whose positions (rune cases) or lists (unique cases) differ"""
    mo = want[0]
    if not np.array_equal(mo, got[0]):
        return [case.names[d] for d in range(len(case.docs)) if int(mo[d + 1] - mo[d]) != int(got[0][d + 1] - got[0][d])
                or not np.array_equal(want[1][int(mo[d]):int(mo[d + 1])], got[1][int(got[0][d]):int(got[0][d + 1])])]
    bad = np.nonzero((want[1] != got[1]) | (want[2] != got[2]))[0]
    return [case.names[d] for d in sorted(set((np.searchsorted(mo, bad, side="right") - 1).tolist()))]


def assert_not_vacuous():
    """-> {wrong reading: the cases (documents) that catch it}.  Counts of cases, evaluated on the CPU; no tolerance"""
    caught = collections.OrderedDict()
    # every byte of the rune cases is a match (so the whole table is compared), and the keywords tie
    for c in small_rune_cases() + [random_documents(), long_document()]:
        mo, ti, po = full_csr(c)
        for d, doc in enumerate(c.docs):
            if not set(doc) & set(NO_MATCH):
                assert set(po[int(mo[d]):int(mo[d + 1])].tolist()) == set(range(len(doc))), (c.name, c.names[d])
        assert c is folded() or (np.diff(po.astype(np.int64)) == 0).any() or len(po) < 2, c.name
    # 1. a decoder that runs on into the neighbouring document, the lead bytes or the slack
    c = document_borders()
    got = map_positions(full_csr(c), tables_unbounded(b"", c.docs, b""))
    caught["decoder crosses a document border"] = differing(c, rune_csr(c), got)
    lead_hits, slack_hits = [], []
    for c in edge_cuts():
        want = rune_csr(c)
        if differing(c, want, map_positions(full_csr(c), tables_unbounded(c.lead, c.docs, b""))):
            lead_hits.append(c.name)
        if differing(c, want, map_positions(full_csr(c), tables_unbounded(b"", c.docs, c.tail + b"\x80" * 8))):
            slack_hits.append(c.name)
    caught["decoder reads the lead bytes"], caught["decoder reads the slack"] = lead_hits, slack_hits
    # 2. to 4.
    for what, table in (("errors=replace grouping", table_replace), ("every 64-byte block a document", table_blocks), ("bytes, not runes", table_bytes)):
        caught[what] = [n for c in small_rune_cases() for n in differing(c, rune_csr(c), rune_csr(c, table))]
    # the forms: each is there, whole and cut
    assert {"two", "three", "four", "two-1", "three-1", "three-2", "four-1", "four-2", "surrogate", "past-10ffff", "f5", "ff", "four+1"} <= set(FORMS)
    assert all("stray-%d" % k in FORMS for k in range(1, 6)) and len(cuts()) >= 40
    assert set(LENGTHS) == {len(d) for d in document_lengths().docs}
    assert len(long_document().docs[1]) > SCAN_TILE * RUNE_BLOCK
    # unique
    c = unique_fixed()
    mo = full_csr(c)[0]
    assert tuple(int(x) for x in np.diff(mo.astype(np.int64))[:len(COUNTS)]) == COUNTS
    lists = unique_lists(full_csr(c))
    assert [len(x) for x, n in zip(lists, c.names) if n.startswith("one term")] == [1]
    assert [len(x) for x, n in zip(lists, c.names) if n.startswith("600 distinct")] == [600, 600]
    caught["lists in term-id order"] = [c.names[d] for d, x in enumerate(lists) if x != sorted(x)]
    rows = unique_rows(ROW_REUSE_DOCS)
    lists = unique_lists(full_csr(rows))
    for g in GRIDS:
        stale = lists_with_stale_rows(lists, g)
        hit = [d for d in range(len(lists)) if stale[d] != lists[d]]
        same = [d for d in range(g, len(lists)) if lists[d] and set(lists[d]).isdisjoint(lists[d - g]) and lists[d - g]]
        assert hit and same, (g, len(hit), len(same))
        caught["row not reset, grid %d" % g] = ["%s[%d]" % (rows.name, d) for d in hit[:3]] + ["... %d documents" % len(hit)]
    for what, names in caught.items():
        assert names, "no case would catch: " + what
    return caught
