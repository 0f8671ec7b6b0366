"""Batches whose SHAPE is the test (test infrastructure: no GPU, no torch): seeded generators and what the oracle says
about them, shared by test_batch_shapes_host.py (which shows that they are what they claim to be) and
test_gpu_batch_shapes.py (which runs them through the kernels).

A. A batch of N = 2^20 + 4 096 + 1 short documents.  launch_exclusive_scan (csrc/gft_kernels.hip) works on tiles of 4 096
   items and k_scan_spine walks the tile totals 256 at a time, so 258 tiles are a second spine round of two tiles, the last
   of one item: the carry between the rounds, partial[n_part] behind a second round and k_scan_final in a block of index
   256 and more run for batches of more than 2^20 items only.  Every document is one of at most 64 pool strings; every
   expectation is computed per pool string and expanded by the batch's index array.

B. Documents that are ONE work unit each with a constructed number and layout of matches, at the limits of k_gather_sorted
   (bucketed rank sort up to 256 matches, tiled rank sort above)."""
import numpy as np

from oracle import dsl_ref
from oracle.pyoracle import Oracle, POS_END, POS_START, pack_strings
from oracle.runes_ref import rune_index_table
from tolower_cases import LENGTH_CHANGERS, ref_lower

POS_MODES = (POS_START, POS_END)

# ---- A. more than 2^20 documents ------------------------------------------------------------------------------------------
SCAN_TILE, SPINE_ROUND = 4096, 256                     # kScanTile, kScanBlock of csrc/gft_kernels.hip
BORDER = SCAN_TILE * SPINE_ROUND                       # 1 048 576 items: the first item of the second spine round
N_BIG = BORDER + SCAN_TILE + 1                         # 258 tiles
EDGE_DOCS = (0, SCAN_TILE - 1, SCAN_TILE, BORDER - 1, BORDER, N_BIG - 1)
RUNE_BLOCK = 64                                        # kRuneBlock
LONG_DOC_LEN = 20000                                   # longer than any work unit (8 192 bytes)

TERMS_A = [b"a", b"ab", b"abc", b"abcde", b"b", b"cab", b"de", b"xy", "é".encode(), b"z"]
EXPRS_A = ['"a" and "b"', 'inord("b" and "a")', 'not "a"', '"xy" or "z" or "de"']

_FIXED_POOL = [
    b"q", b"hhh", b"QRS", b"A", b"mno pqr",                                         # no match
    b"z", b"hq z", b"k xy",                                                         # one match
    b"abab", b"abcde", b"cabcab", b"zz", b"dede de", b"ba",                         # several, terms repeated
    "ñab".encode(), "€abc".encode(), "ñ€xy z".encode(),         # 2- and 3-byte runes in front of a match
    "café de".encode(), "ééb".encode(),
    "Éab".encode(), "À xy".encode(),                                      # upper-case Latin-1
    chr(LENGTH_CHANGERS[1]).encode() + b"a", chr(LENGTH_CHANGERS[0]).encode() + b"b",   # lower-case form is shorter ...
    chr(LENGTH_CHANGERS[-1]).encode() + b"z",                                       # ... and longer
    b"a\xffb", b"\x80xy", b"ab\xc3",                                                # invalid bytes (the last: a lead byte cut off)
    b"ABC ab",
]


def pool():
    """the distinct documents: the hand-made ones, seeded random ones up to 63, and the empty one LAST"""
    rng = np.random.default_rng(20261018)
    out = list(_FIXED_POOL)
    alpha = b"abcdexyz q"
    while len(out) < 63:
        s = bytes(alpha[i] for i in rng.integers(0, len(alpha), int(rng.integers(1, 13))))
        if s not in out:
            out.append(s)
    assert all(1 <= len(s) <= 12 for s in out)
    return out + [b""]


def _ragged(rows, dtype):
    """list of 1-d sequences -> (matrix [n, max len] padded with zeros, lengths)"""
    lens = np.asarray([len(r) for r in rows], np.int64)
    m = np.zeros((len(rows), max(int(lens.max()), 1)), dtype)
    for i, r in enumerate(rows):
        m[i, :len(r)] = np.frombuffer(r, np.uint8) if isinstance(r, bytes) else r
    return m, lens


def expand(rows, idx, dtype):
    """the rows picked by idx, one behind the other -> (flat array, offsets u64 [len(idx) + 1]); numpy only"""
    m, lens = _ragged(rows, dtype)
    off = np.zeros(len(idx) + 1, np.uint64)
    np.cumsum(lens[idx], out=off[1:])
    flat = m[idx][np.arange(m.shape[1])[None, :] < lens[idx][:, None]]
    return np.ascontiguousarray(flat), off


def index_array(variant):
    """which pool string each of the N_BIG documents is.  "full": every document non-empty, the documents at the tile and
    round borders hold matches, runes and a letter to lower-case; "holes": about a third of the documents empty, those
    at the borders among them"""
    rng = np.random.default_rng(7)
    p = pool()
    idx = rng.integers(0, len(p) - 1, N_BIG)
    for k, d in enumerate(EDGE_DOCS):
        idx[d] = p.index(("ñ€xy z".encode(), "Éab".encode(), b"cabcab")[k % 3])
    if variant == "holes":
        empty = rng.random(N_BIG) < 1.0 / 3
        empty[list(EDGE_DOCS)] = True
        idx[empty] = len(p) - 1
    else:
        assert variant == "full"
    return idx


def programs(exprs, term_id, n_terms, case_sensitive=True):
    """expression strings -> postfix words for Engine.set_programs (helpers.tree_to_program), every literal a dictionary term"""
    from helpers import tree_to_program

    def slot_of(lit):
        t = term_id(lit)
        assert 0 <= t < n_terms, lit
        return t
    return [tree_to_program(dsl_ref.parse(e, case_sensitive)[0], slot_of) for e in exprs]


class Expected:
    """what the oracle says about every pool string, and the expansion of it over an index array"""

    def __init__(self):
        self.pool = p = pool()
        blob, off = pack_strings(p)
        self.csr = {}
        for mode in POS_MODES:
            o = Oracle(TERMS_A, mode)
            mo, ti, po = o.scan(blob, off)
            self.csr[mode] = [(ti[int(mo[i]):int(mo[i + 1])], po[int(mo[i]):int(mo[i + 1])]) for i in range(len(p))]
        o = Oracle(TERMS_A, POS_START)
        o.set_expressions(EXPRS_A, True)
        self.bitmap_rows = o.process(blob, off)
        self.unique_rows = [np.asarray(list(dict.fromkeys(t.tolist())), np.uint32) for t, _ in self.csr[POS_START]]
        self.rune_rows = [np.asarray([rune_index_table(s)[int(x)] for x in pp], np.uint32) for s, (_, pp) in zip(p, self.csr[POS_START])]
        self.lower_rows = [ref_lower(s) for s in p]

    def text(self, idx):
        """-> (blob u8, doc_off u64)"""
        return expand(self.pool, idx, np.uint8)

    def scan(self, idx, mode):
        ti, off = expand([t for t, _ in self.csr[mode]], idx, np.uint32)
        po, _ = expand([q for _, q in self.csr[mode]], idx, np.uint32)
        return off, ti, po

    def unique(self, idx):
        ti, off = expand(self.unique_rows, idx, np.uint32)
        return off, ti, np.zeros(ti.size, np.uint32)

    def runes(self, idx):
        off, ti, _ = self.scan(idx, POS_START)
        return off, ti, expand(self.rune_rows, idx, np.uint32)[0]

    def lower(self, idx):
        """-> (bytes u8, offsets u64)"""
        return expand(self.lower_rows, idx, np.uint8)

    def bitmap(self, idx):
        return np.ascontiguousarray(self.bitmap_rows[idx])

    def rune_blocks(self, idx):
        """per document: its 64-byte blocks (k_rune_doc_blocks)"""
        lens = np.asarray([len(s) for s in self.pool], np.int64)[idx]
        return (lens + RUNE_BLOCK - 1) // RUNE_BLOCK


def long_document():
    """LONG_DOC_LEN bytes with matches all along: more than one work unit"""
    rng = np.random.default_rng(99)
    alpha = b"abcdexyz q"
    return bytes(alpha[i] for i in rng.integers(0, len(alpha), LONG_DOC_LEN))


def with_long_document(blob, off, at):
    """the batch with document `at` replaced by long_document() -> (blob, doc_off)"""
    doc = np.frombuffer(long_document(), np.uint8)
    a, b = int(off[at]), int(off[at + 1])
    off2 = off.copy()
    off2[at + 1:] += np.uint64(doc.size - (b - a))
    return np.concatenate([blob[:a], doc, blob[b:]]), off2


# ---- B. units at the limits of k_gather_sorted ----------------------------------------------------------------------------
FIFO, UNIT_MAX, BINS = 256, 8192, 256                  # kScan2FifoCap, kScan2UnitMax, kSortBins
EXACT_COUNTS = list(range(250, 263)) + list(range(508, 517)) + [768, 769]
UNIT_LENGTHS = [255, 256, 257, 511, 512, 513, 8191, 8192]


def run_matches(doc, kmax):
    """matches of the dictionary {a^1 .. a^kmax, b} in doc, by arithmetic: a run of r `a` has min(e, kmax) matches ending at its
    e-th byte, every `b` is one"""
    n = r = 0
    for c in doc:
        r = r + 1 if c == 0x61 else 0
        n += min(r, kmax) + (1 if c == 0x62 else 0)
    return n


def _embed(run, at, size=UNIT_MAX):
    assert at + len(run) <= size
    return b"x" * at + run + b"x" * (size - at - len(run))


class Family:
    """one dictionary, documents of one work unit each (but for `cut`), the constructed number of matches per document"""

    def __init__(self, name, terms, kmax, docs, seed):
        self.name, self.terms, self.kmax = name, terms, kmax
        rng = np.random.default_rng(seed)
        docs = list(docs)
        docs += [b""] * (len(docs) // 2 + 2)                              # empty documents in between
        self.texts = [docs[i] for i in rng.permutation(len(docs))]
        self.counts = [run_matches(t, kmax) for t in self.texts]

    def packed(self):
        return pack_strings(self.texts)

    def oracle(self, mode):
        return Oracle(self.terms, mode)

    def unique_of(self, csr):
        """a scan's CSR -> every term once per document, first occurrences in order, positions 0"""
        mo, ti, _ = csr
        rows = [list(dict.fromkeys(ti[int(mo[d]):int(mo[d + 1])].tolist())) for d in range(len(self.texts))]
        off = np.zeros(len(rows) + 1, np.uint64)
        off[1:] = np.cumsum([len(r) for r in rows])
        flat = np.asarray([t for r in rows for t in r], np.uint32)
        return off, flat, np.zeros(flat.size, np.uint32)


def _exact_doc(c):
    """the shortest document over {a, aa, b} with c matches: "a" * L + "b" * m has 2 L - 1 + m.  (256 bytes hold 511 matches
    of this dictionary at most: the documents for 512 and more are longer, up to 385 bytes)"""
    L = (c + 1) // 2
    return b"a" * L + b"b" * (c - (2 * L - 1))


def family_exact():
    """dictionary {a, aa, b}: every count around 256, 512 and 768, as a document of its own (one bin per end offset up to
    256 bytes) and as the same run inside 8 192 bytes of filler (bins of 32 end offsets); a second way to the counts around
    256 with more `b` (matches of ONE term in a row); documents of the lengths at which `own >> shift` changes, matches
    at their first and last bytes; 8 193 and 16 385 bytes: two and three units, cut inside a run"""
    rng = np.random.default_rng(3)
    docs = []
    for c in EXACT_COUNTS:
        run = _exact_doc(c)
        assert run_matches(run, 2) == c
        docs += [run, _embed(run, int(rng.integers(0, UNIT_MAX - len(run) + 1)))]
    for c in (255, 256, 257):
        docs.append(b"a" * 100 + b"b" * (c - 199))
    for n in UNIT_LENGTHS:
        mid = bytearray(b"x" * (n - 5))
        for at in rng.integers(0, n - 5, 12):
            mid[int(at)] = 0x61
        docs.append(b"ab" + bytes(mid) + b"baa")
    d = bytearray(b"x" * 8193)
    d[4077:4117] = b"a" * 40                                                    # (units [0, 4 097) and [4 097, 8 193))
    d[0:1], d[8192:8193] = b"b", b"a"
    docs.append(bytes(d))
    d = bytearray(b"x" * 16385)
    for border in (5462, 10924):                                                # (three units of 5 462 bytes, the last 5 461)
        d[border - 150:border + 150] = b"a" * 300
    d[16384:16385] = b"b"
    docs.append(bytes(d))
    return Family("exact", [b"a", b"aa", b"b"], 2, docs, 11)


def family_onebin():
    """dictionary {a^1 .. a^16, b}: a run of 23 `a` is 248 matches, 7 / 8 / 9 `b` behind it make 255 / 256 / 257 inside 32 bytes:
    at a 32-aligned offset of an 8 192-byte document all of them fall into ONE bin (cmax = n), 16 bytes on into two"""
    docs = []
    for nb in (7, 8, 9):
        run = b"a" * 23 + b"b" * nb
        assert run_matches(run, 16) == 248 + nb
        for at in (0, 32 * 100, UNIT_MAX - 32, 32 * 57 + 16, 32 * 200 + 16):
            docs.append(_embed(run, at))
        docs.append(run)
    return Family("onebin", [b"a" * k for k in range(1, 17)] + [b"b"], 16, docs, 12)


def family_ties():
    """dictionary {a^1 .. a^64}: up to 64 matches end at one byte and only the length orders them.  "a" * 70 is 2 464 matches
    (tiled path); "a" * 22 is 253 (bucketed path), alone and in one and in two bins of a long document"""
    docs = [b"a" * 70, _embed(b"a" * 70, 4000), b"a" * 22, _embed(b"a" * 22, 32 * 9), _embed(b"a" * 22, 32 * 9 + 20), b"a" * 23]
    return Family("ties", [b"a" * k for k in range(1, 65)], 64, docs, 13)


def family_ties200():
    """dictionary {a^1 .. a^200} over "a" * 256: 200 * 256 - 19 900 = 31 300 matches in one unit, 123 tiles of the tiled path"""
    docs = [b"a" * 256, b"a" * 3, b"xaax"]
    return Family("ties200", [b"a" * k for k in range(1, 201)], 200, docs, 14)


GATHER_WAVES_PER_CU = 4 * 16  # k_gather_sorted's grid is capped at 16 blocks of 4 waves per CU
INTERLEAVE_DOCS = 24000       # non-empty ones, a unit each: more than the gather has waves on 256 CUs (the GPU test checks its own device)


def family_interleave():
    """dictionary {a, aa, b}, tens of thousands of small documents of 259 (tiled path), 255 and 256 (bucketed, full) and 6
    matches in random order: the gather's grid is capped, so a wave takes several units one after the other and a
    bucketed unit finds the LDS rows as a tiled one left them"""
    rng = np.random.default_rng(5)
    kinds = [b"a" * 130, b"a" * 128, b"a" * 128 + b"b", b"aaab", b"b"]
    docs = [kinds[int(k)] for k in rng.integers(0, len(kinds), INTERLEAVE_DOCS)]
    return Family("interleave", [b"a", b"aa", b"b"], 2, docs, 15)


FAMILIES = {"exact": family_exact, "onebin": family_onebin, "ties": family_ties, "ties200": family_ties200,
            "interleave": family_interleave}
