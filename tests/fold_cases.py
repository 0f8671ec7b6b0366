"""Where in the text a violation of the fold-safety rule lies (test infrastructure: numpy only, no GPU, nothing of the product
loaded; no tests in here).  gft_last_nonascii is decided by four pieces of code that share a rule and no code path -- k_fold_safe
with k_fold_doc_edges (16-byte blocks aligned in memory), gft_scan3 (pieces at r * 1024 + lane * 16 from the unit's first byte),
gft_scan5 over a small alphabet (pieces at lane * C + q * 16, every piece of a lane that saw a high byte) and gft_scan5 over a
large one (the same pieces, listed one by one).  This module puts every kind of violation, and every safe pair, at every byte
position around every border those geometries have, in documents whose lengths give scan5 every lane width C.

The reference is the contract of include/gft.h at gft_last_nonascii, restated: a document is safe iff it consists of ASCII and of
the pairs C2 80..BF, C3 9F..BF and C3 97 (`rows_safe`).  Expected verdicts come from it alone.  The Python model of the kernels'
geometries further down (`model_verdict`) serves assert_not_vacuous() and nothing else: it says which piece byte, which trip of
the job list and which wrong reading of the rule a case reaches, so that the lists provably hold the cases they were made for.

Shared by test_fold_cases_host.py (the lists are what they claim, the rule is what the product needs) and
test_gpu_fold_verdict.py (the kernels)."""
import collections
import functools

import numpy as np

UNIT_MAX = 8192                                  # bytes per work unit of gft_scan3 and of gft_scan5 behind sparse batches
LENGTHS = (40, 700, 1000, 1100, 2048, 3000, 6000, 8192, 8193, 20000)
FULL = (1000, 1100, 8192, 20000)                 # swept at every landmark; the others at the document's start and end
SCAN5_C = {40: 4, 700: 12, 1000: 16, 1100: 20, 2048: 32, 3000: 48, 6000: 96, 8192: 128}      # one unit: bytes per lane
FILLERS = ("ascii", "dense")
WINDOW = 36                                      # every residue modulo 16 and modulo every C up to 32, on both sides of a border
FREE_WINDOW = 16
LEAD, SLACK = 16, 64                             # bytes in front of the first document (doc_off[0] != 0) and behind the last

# ---- kinds -----------------------------------------------------------------------------------------------------------------
SENSITIVE = collections.OrderedDict((k, bytes.fromhex(v)) for k, v in [
    ("C3 89", "c389"), ("C3 80", "c380"), ("C3 9E", "c39e"), ("C3 96", "c396"), ("C3 98", "c398"),      # upper-case Latin-1
    ("C3 'a'", "c361"), ("C2 'a'", "c261"),                                                             # a lead that nothing continues
    ("C3 C3 A9", "c3c3a9"), ("C2 C2 A0", "c2c2a0"),                                                     # a lead behind a lead
    ("'a' A9", "61a9"), ("'a' 80", "6180"), ("'a' BF", "61bf"),                                         # a continuation byte with no lead
    ("C3 A9 A9", "c3a9a9")])
FREE = collections.OrderedDict((k, bytes.fromhex(v)) for k, v in [
    ("C4 B0", "c4b0"), ("C5 BF", "c5bf"), ("E2 84 AA", "e284aa"), ("F0 9F 98 80", "f09f9880"), ("FF", "ff"), ("C0 80", "c080"),
    ("C1 BF", "c1bf"), ("F5", "f5")])
RIM_END = collections.OrderedDict([("lone C3 at the end", b"\xc3"), ("lone C2 at the end", b"\xc2")])
RIM_START = collections.OrderedDict([("A9 at the start", b"\xa9"), ("80 at the start", b"\x80"), ("BF at the start", b"\xbf")])
SAFE_PAIRS = collections.OrderedDict((k, bytes.fromhex(v)) for k, v in [
    ("C2 80", "c280"), ("C2 BF", "c2bf"), ("C3 9F", "c39f"), ("C3 97", "c397"), ("C3 BF", "c3bf"), ("C3 A9", "c3a9"),
    # (beyond the six pairs: two pairs back to back -- the second lead stands behind a continuation byte -- so that the safe
    # cases are not outnumbered)
    ("C3 9F C3 97", "c39fc397"), ("C2 80 C3 BF", "c280c3bf")])
VIOLATIONS = collections.OrderedDict(list(SENSITIVE.items()) + list(FREE.items()) + list(RIM_END.items()) + list(RIM_START.items()))

Case = collections.namedtuple("Case", "doc kind p")          # doc: index into the family's offsets; p: the kind's first byte


# ---- the reference ---------------------------------------------------------------------------------------------------------
def rows_safe(rows):
    """the contract for documents of one length, one per row of a uint8 array -> bool per row.  Restated without a walk: every
    high byte is C2, C3 or a continuation byte, every lead is followed -- inside the document -- by a continuation byte, every
    continuation byte stands behind a lead, and behind C3 it is 9F..BF or 97.  (Leads and continuation bytes are disjoint, so a
    byte has one role and the pairs cannot overlap.)"""
    a = np.atleast_2d(np.asarray(rows, dtype=np.uint8))
    lead = (a == 0xC2) | (a == 0xC3)
    cont = (a & 0xC0) == 0x80
    bad = ((a >= 0x80) & ~lead & ~cont).any(axis=1)
    if a.shape[1]:
        bad |= lead[:, -1] | cont[:, 0]
        bad |= (lead[:, :-1] & ~cont[:, 1:]).any(axis=1) | (cont[:, 1:] & ~lead[:, :-1]).any(axis=1)
        nxt = a[:, 1:]
        bad |= ((a[:, :-1] == 0xC3) & cont[:, 1:] & ~((nxt >= 0x9F) | (nxt == 0x97))).any(axis=1)
    return ~bad


def doc_safe(doc):
    return bool(rows_safe(np.frombuffer(bytes(doc), dtype=np.uint8).reshape(1, -1))[0])


def ascii_fold(doc):
    """the scan kernels' fold: A-Z and nothing else"""
    a = np.frombuffer(bytes(doc), dtype=np.uint8)
    return np.where((a >= 65) & (a <= 90), a + 32, a).astype(np.uint8).tobytes()


# ---- the units and the pieces ----------------------------------------------------------------------------------------------
def unit_slices(n, unit_max=UNIT_MAX):
    """unit_slice of gft_kernels.hpp for a document of n bytes -> [(lo, hi)]: k = ceil(n / unit_max) units (one for n <= unit_max)
    of per = ceil(n / k) bytes, the last one shorter"""
    k = 1 if n <= unit_max else (n + unit_max - 1) // unit_max
    per = min((n + k - 1) // k, unit_max)
    return [(min(i * per, n), min(i * per + per, n)) for i in range(k)]


def scan5_c(own):
    """gft_scan5.hip: bytes per lane of a unit of `own` bytes (a multiple of 4, at most 128)"""
    return ((own + 63) // 64 + 3) & ~3


# ---- fillers ---------------------------------------------------------------------------------------------------------------
_LETTERS = np.frombuffer(b"xqzj XQZJ  ", dtype=np.uint8)         # no keyword of the tests' dictionaries is spelt with these
_PAIR = b"\xc3\xa9"


@functools.lru_cache(maxsize=None)
def _ascii_base(n):
    rng = np.random.default_rng([20261020, n])
    return _LETTERS[rng.integers(0, len(_LETTERS), n)]


def build_doc(n, filler, p, v):
    """a document of n bytes of `filler` with the bytes v at p.  dense: C3 A9 back to back, one ASCII byte in front of v when p
    is odd and one behind it when an odd number of bytes is left"""
    v = np.frombuffer(bytes(v), dtype=np.uint8)
    assert 0 <= p and p + len(v) <= n
    if filler == "ascii":
        d = _ascii_base(n).copy()
        d[p:p + len(v)] = v
        return d
    d = np.frombuffer(_PAIR * (n // 2 + 1), dtype=np.uint8)[:n].copy()
    if p & 1:
        d[p - 1] = ord("x")
    d[p:p + len(v)] = v
    s = p + len(v)
    if (n - s) & 1:
        d[s] = ord("j")
        s += 1
    d[s:] = np.frombuffer(_PAIR * ((n - s) // 2), dtype=np.uint8)
    return d


def spacer(s):
    """a safe document of s >= 2 bytes between two cases: it begins with a pair (what a piece that reads past its document's end
    sees) and moves the next case to another residue of the 16-byte grid"""
    return np.frombuffer(_PAIR * (s // 2) + b"x" * (s & 1), dtype=np.uint8)


# ---- landmarks -------------------------------------------------------------------------------------------------------------
def borders(n):
    """name -> offset of every border inside a document of n bytes that one of the judges has"""
    out = collections.OrderedDict()
    units = unit_slices(n)
    for i, (lo, _) in enumerate(units[1:]):
        out["unit %d" % (i + 1)] = lo
    if n > 1024:
        out["round 1"] = 1024
    c = scan5_c(units[0][1] - units[0][0])
    for lane in (1, 31, 63):
        if lane * c < units[0][1]:
            out["lane %d" % lane] = lane * c
    return out


def positions(n, vlen, full, window=WINDOW):
    """the first bytes at which a kind of vlen bytes is placed: `window` consecutive positions at the document's start, at its
    end (the last of them puts the kind's last byte on the document's last byte) and, for a full sweep, around every border"""
    last = n - vlen
    ps = set(range(0, min(window, last + 1))) | set(range(max(0, last - window + 1), last + 1))
    if full:
        for b in borders(n).values():
            ps |= set(range(b - window // 2, b + window // 2))
    return sorted(p for p in ps if 0 <= p <= last)


def free_positions(n, vlen):
    b = borders(n)["lane 31"]
    return [p for p in range(b - FREE_WINDOW // 2, b + FREE_WINDOW // 2) if 0 <= p <= n - vlen]


# ---- families --------------------------------------------------------------------------------------------------------------
class Family:
    """documents of one (length, filler) in ONE blob: LEAD bytes of C3 in front (doc_off[0] != 0), then case, spacer, case,
    spacer ..., then SLACK bytes of 89.  cases[i].doc indexes off; unsafe[i] is the reference's word on that document.  The blob
    is 16-byte aligned in the tests (a fresh allocation), so a document's residue on the 16-byte grid is off[d] % 16"""

    def __init__(self, name, docs, cases):
        self.name, self.cases = name, cases
        lens = np.asarray([len(d) for d in docs], dtype=np.uint64)
        self.off = np.zeros(len(docs) + 1, dtype=np.uint64)
        self.off[0] = LEAD
        self.off[1:] = LEAD + np.cumsum(lens, dtype=np.uint64)
        self.blob = np.concatenate([np.full(LEAD, 0xC3, np.uint8)] + docs + [np.full(SLACK, 0x89, np.uint8)])
        self.n_docs = len(docs)
        self.unsafe = np.zeros(len(cases), dtype=bool)
        by_len = collections.defaultdict(list)
        for i, c in enumerate(cases):
            by_len[len(docs[c.doc])].append(i)
        for idx in by_len.values():                          # (the reference, a length at a time)
            self.unsafe[idx] = ~rows_safe(np.stack([docs[cases[i].doc] for i in idx]))
        for a in (self.off, self.blob, self.unsafe):
            a.setflags(write=False)

    def doc(self, d):
        return self.blob[int(self.off[d]):int(self.off[d + 1])]

    def span(self, d):
        return int(self.off[d]), int(self.off[d + 1])


def doc_safe_np(a):
    return bool(rows_safe(a.reshape(1, -1))[0])


def _interleave(name, n, made):
    """made: [(kind, p, document)] -> a Family with a spacer behind every case.  Spacer lengths are drawn so that the cases start
    at every residue of the 16-byte grid whatever n is"""
    rng = np.random.default_rng([20261021, n, len(made)])
    docs, cases = [], []
    for kind, p, d in made:
        cases.append(Case(len(docs), kind, p))
        docs.append(d)
        docs.append(spacer(int(rng.integers(2, 18))))
    return Family(name, docs, cases)


@functools.lru_cache(maxsize=None)
def unsafe_family(n, filler):
    """every violation of every kind in documents of n bytes, one per document"""
    full = n in FULL
    made = []
    for kind, v in SENSITIVE.items():
        made += [(kind, p, build_doc(n, filler, p, v)) for p in positions(n, len(v), full)]
    if full:
        for kind, v in FREE.items():
            made += [(kind, p, build_doc(n, filler, p, v)) for p in free_positions(n, len(v))]
    for kind, v in RIM_END.items():
        made.append((kind, n - 1, build_doc(n, filler, n - 1, v)))
    for kind, v in RIM_START.items():
        made.append((kind, 0, build_doc(n, filler, 0, v)))
    return _interleave("unsafe %d %s" % (n, filler), n, made)


@functools.lru_cache(maxsize=None)
def safe_family(n, filler):
    """the same sweeps with a safe pair in place of the violation: pairs cut by pieces, lanes, rounds and units, never by a
    document; at p = 0 and at the last position the document begins / ends with a whole pair"""
    full = n in FULL
    made = []
    for kind, v in SAFE_PAIRS.items():
        made += [(kind, p, build_doc(n, filler, p, v)) for p in positions(n, len(v), full)]
    return _interleave("safe %d %s" % (n, filler), n, made)


RIM_LENGTHS = tuple(range(17, 33)) + tuple(range(1000, 1016))        # every residue modulo 16, below and above one piece


@functools.lru_cache(maxsize=None)
def rim_family(filler):
    """the two violations that exist only at a document's rim, in documents of every length modulo 16 that follow each other
    WITHOUT a spacer: a document that ends in a lone lead is followed by one that begins with a continuation byte, so that across
    the border stands a pair which the rule accepts -- and strings.ToLower, which sees documents one by one, does not"""
    docs, cases = [], []
    for rep in range(2):                                     # (twice: the second round starts at other residues)
        for n in RIM_LENGTHS:
            for (ke, ve), (ks, vs) in [(e, s) for e in RIM_END.items() for s in RIM_START.items()]:
                cases.append(Case(len(docs), ke, n - 1))
                docs.append(build_doc(n, filler, n - 1, ve))
                cases.append(Case(len(docs), ks, 0))
                docs.append(build_doc(n, filler, 0, vs))
        docs.append(spacer(3))
    return Family("rim %s" % filler, docs, cases)


UNSAFE_FAMILIES = [("unsafe", n, f) for n in LENGTHS for f in FILLERS] + [("rim", 0, f) for f in FILLERS]
SAFE_FAMILIES = [("safe", n, f) for n in LENGTHS for f in FILLERS]


def family(which, n, filler):
    return unsafe_family(n, filler) if which == "unsafe" else safe_family(n, filler) if which == "safe" else rim_family(filler)


def family_id(key):
    return "%s-%d-%s" % key if key[0] != "rim" else "rim-%s" % key[2]


def thinned(n, filler):
    """the cases of unsafe_family(n, filler) for the other ways a batch is scanned: every context-sensitive kind with its first
    byte on bytes 0 and 15 of a 16-byte piece, on both sides of the first unit border, and with its last byte on the document's"""
    fam = unsafe_family(n, filler)
    units = unit_slices(n)
    want = {borders(n)["lane 31"] // 16 * 16, borders(n)["lane 31"] // 16 * 16 + 15}
    if len(units) > 1:
        want |= {units[1][0] - 1, units[1][0]}
    out = []
    for i, c in enumerate(fam.cases):
        if c.kind in SENSITIVE and (c.p in want or c.p == n - len(SENSITIVE[c.kind])):
            out.append(i)
    return fam, out


# ---- the model of the judges (assert_not_vacuous only) -----------------------------------------------------------------------
READINGS = ("jnext taken as a continuation byte", "jprev taken as 0 everywhere", "jprev not zeroed at a document's start",
            "doc_left ignored", "k_hi taken as 16", "the last trip dropped", "C3 80..9E accepted", "C3 97 refused",
            "the document-edge kernel skipped")
JUDGES = ("scan3", "scan5-small", "scan5-large", "k_fold_safe")


def _pair_bad(p, b, reading):
    """a continuation byte b behind p"""
    p_lead = p in (0xC2, 0xC3)
    if not p_lead:
        return True
    if p != 0xC3:
        return False
    if reading == "C3 80..9E accepted":
        return False
    if reading == "C3 97 refused":
        return b < 0x9F
    return not (b >= 0x9F or b == 0x97)


_PIECES = {}


def piece_unsafe(w, jprev, jnext, k_hi, doc_left, reading=None):
    """fold_piece_unsafe of gft_foldsafe_dev.hpp on the 16 bytes w (remembered: the dense documents repeat their pieces)"""
    key = (w.tobytes(), jprev, jnext, k_hi, min(doc_left, 17), reading)
    if key not in _PIECES:
        _PIECES[key] = _piece_unsafe(w, jprev, jnext, k_hi, doc_left, reading)
    return _PIECES[key]


def _piece_unsafe(w, jprev, jnext, k_hi, doc_left, reading):
    bad = False
    for k in range(min(k_hi, 16)):
        b = int(w[k])
        if b < 0x80:
            continue
        p = int(w[k - 1]) if k else jprev
        if b in (0xC2, 0xC3):
            nb = int(w[k + 1]) if k + 1 < 16 else jnext
            bad |= p in (0xC2, 0xC3) or (nb & 0xC0) != 0x80 or k + 1 >= doc_left
        elif (b & 0xC0) == 0x80:
            bad |= _pair_bad(p, b, reading)
        else:
            bad = True
    return bad


@functools.lru_cache(maxsize=None)
def _scan5_grid(own):
    """-> (C, offsets of scan5's pieces [q, lane] -- the list's order --, which of them hold a byte of the unit)"""
    c = scan5_c(own)
    npieces = (c // 4 + 3) // 4
    lane, q = np.meshgrid(np.arange(64), np.arange(npieces))
    nvalid = np.clip(own - lane * c, 0, c)
    return c, lane * c + q * 16, q * 16 < nvalid


def unit_jobs(blob, judge, ua, own):
    """the pieces (offsets from the unit's first byte at blob offset ua) that the kernel lists for a unit, in list order: scan3 by
    (round, lane), scan5 by (q, lane)"""
    if judge == "scan3":
        hi = (blob[ua:ua + (own + 15) // 16 * 16] & 0x80) != 0
        return np.unique(np.nonzero(hi)[0] // 16 * 16).tolist()
    c, start, valid = _scan5_grid(own)
    seg = blob[ua:ua + 64 * c + 48]
    hb = np.zeros(64 * c + 48, dtype=np.int64)
    hb[:len(seg)] = (seg & 0x80) != 0
    cs = np.concatenate([[0], np.cumsum(hb)])
    high = valid & ((cs[start + 16] - cs[start]) > 0)
    listed = high if judge == "scan5-large" else valid & high.any(axis=0)[None, :]
    return [int(x) for x in start[listed]]


def model_verdict(blob, lo, hi, judge, reading=None, trace=None):
    """what `judge` would say of the document blob[lo, hi) were its code read as `reading` (None: as it stands).  trace, a list,
    receives (unit, job index, jobs in the unit, offset of the piece in the document) of every piece judged"""
    if judge == "k_fold_safe":
        return _model_fold_safe(blob, lo, hi, reading)
    bad = False
    for u, (ulo, uhi) in enumerate(unit_slices(hi - lo)):
        ua, own = lo + ulo, uhi - ulo
        jobs = unit_jobs(blob, judge, ua, own)
        n = len(jobs)
        for i, rel in enumerate(jobs):
            if reading == "the last trip dropped" and i // 64 == (n - 1) // 64:
                continue
            a = ua + rel
            jprev = int(blob[a - 1]) if a and (rel or ulo) else 0
            if reading == "jprev not zeroed at a document's start" and a:
                jprev = int(blob[a - 1])
            if reading == "jprev taken as 0 everywhere":
                jprev = 0
            jnext = 0x80 if reading == "jnext taken as a continuation byte" else int(blob[a + 16])
            k_hi = 16 if reading == "k_hi taken as 16" else min(own - rel, 16)
            doc_left = 1 << 30 if reading == "doc_left ignored" else min(hi - a, 255)
            if trace is not None:
                trace.append((u, i, n, ulo + rel))
            bad |= piece_unsafe(blob[a:a + 16], jprev, jnext, k_hi, doc_left, reading)
    return bad


def _model_fold_safe(blob, lo, hi, reading, off=None):
    """k_fold_safe over [lo, hi) and k_fold_doc_edges for the documents at the offsets `off` (None: the one document)"""
    bad = False
    highs = np.nonzero((blob[lo:hi] & 0x80) != 0)[0] + lo
    after = highs[(highs % 16 == 15) & (highs + 1 < hi)]                      # (a lead that ends a block is judged by the next block)
    for blk in np.unique(np.concatenate([highs // 16 * 16, after // 16 * 16 + 16])).tolist():
        prev = int(blob[blk - 1]) if blk > lo else 0
        k_lo, k_hi = max(lo - blk, 0), min(hi - blk, 16)
        key = (blob[blk:blk + 16].tobytes(), prev, k_lo, k_hi, blk + k_hi == hi, reading)
        if key not in _PIECES:
            _PIECES[key] = _block_unsafe(*key)
        bad |= _PIECES[key]
    if reading != "the document-edge kernel skipped":
        off = [lo, hi] if off is None else off
        for a, b in zip(off[:-1], off[1:]):
            bad |= b > a and ((int(blob[a]) & 0xC0) == 0x80 or int(blob[b - 1]) in (0xC2, 0xC3))
    return bad


def _block_unsafe(w, prev, k_lo, k_hi, ends, reading):
    """one thread of k_fold_safe: the bytes [k_lo, k_hi) of the 16-byte block w; ends: the text ends with the block's byte k_hi - 1"""
    bad = prev in (0xC2, 0xC3) and k_lo == 0 and w[0] < 0x80
    for k in range(k_lo, k_hi):
        b = w[k]
        if b < 0x80:
            continue
        p = w[k - 1] if k > k_lo else (prev if k == 0 else 0)
        if b in (0xC2, 0xC3):
            bad |= p in (0xC2, 0xC3)
            if k + 1 < k_hi:
                bad |= (w[k + 1] & 0xC0) != 0x80
            elif ends:
                bad = True
        elif (b & 0xC0) == 0x80:
            bad |= _pair_bad(p, b, reading)
        else:
            bad = True
    return bad


def model_batch_verdict(blob, off, judge, reading=None):
    """model_verdict for the batch of documents at the offsets `off`: the OR over the documents, and for k_fold_safe one pass
    over the whole range, which sees no border"""
    off = [int(x) for x in off]
    if judge == "k_fold_safe":
        return _model_fold_safe(blob, off[0], off[-1], reading, off)
    return any(model_verdict(blob, a, b, judge, reading) for a, b in zip(off[:-1], off[1:]))


def rim_pairs(filler):
    """-> (family, [d]): the batches of TWO documents (d, d + 1) of rim_family in which the first ends in a lone lead, the second
    begins with a continuation byte, and the rule accepts the pair across the border: nothing but the look at the documents'
    own first and last bytes makes such a batch unsafe"""
    fam = rim_family(filler)
    out = []
    for c in fam.cases:
        if c.kind in RIM_END and doc_safe(bytes(fam.doc(c.doc)[-1:]) + bytes(fam.doc(c.doc + 1)[:1])):
            out.append(c.doc)
    return fam, out


def covering(n, judge, p):
    """-> [(unit, byte of the piece)] for every piece of `judge`'s geometry that covers byte p of a document of n bytes"""
    out = []
    for u, (ulo, uhi) in enumerate(unit_slices(n)):
        if not ulo <= p < uhi:
            continue
        r, own = p - ulo, uhi - ulo
        if judge == "scan3":
            out.append((u, r % 16))
            continue
        c = scan5_c(own)
        for lane in range(max(0, r // c - 1), r // c + 1):
            nvalid = min(max(own - lane * c, 0), c)
            for q in range((c // 4 + 3) // 4):
                if q * 16 < nvalid and lane * c + q * 16 <= r < lane * c + q * 16 + 16:
                    out.append((u, r - lane * c - q * 16))
    return out


def n_single_cases():
    """(unsafe, safe) documents that the GPU tests scan one at a time"""
    bad = sum(int(family(*k).unsafe.sum()) for k in UNSAFE_FAMILIES)
    good = sum(len(family(*k).cases) for k in SAFE_FAMILIES)
    return bad, good


def assert_not_vacuous(log=None):
    """conditions on the inputs, all evaluated on the CPU.  log, a dict, receives which case shows each wrong reading"""
    log = {} if log is None else log
    # the labels are the reference's: every violation makes its document unsafe, every safe sweep is safe, spacers included
    for key in UNSAFE_FAMILIES:
        fam = family(*key)
        assert fam.unsafe.all(), (fam.name, [fam.cases[i] for i in np.nonzero(~fam.unsafe)[0][:5]])
        assert all(doc_safe_np(fam.doc(c.doc + 1)) for c in fam.cases[:40] if key[0] == "unsafe")
        assert {int(fam.off[c.doc]) % 16 for c in fam.cases} == set(range(16)), fam.name
    for key in SAFE_FAMILIES:
        fam = family(*key)
        assert not fam.unsafe.any(), fam.name
        assert rows_safe(fam.blob[LEAD:int(fam.off[-1])].reshape(1, -1))[0], fam.name          # (no border between two documents cuts a pair)
        assert {int(fam.off[c.doc]) % 16 for c in fam.cases} == set(range(16)), fam.name
        heads = {bytes(fam.doc(c.doc)[:2]) for c in fam.cases if c.p == 0}
        tails = {bytes(fam.doc(c.doc)[-2:]) for c in fam.cases if c.p + len(SAFE_PAIRS[c.kind]) == key[1]}
        assert {bytes(v[:2]) for v in SAFE_PAIRS.values()} <= heads and {bytes(v[-2:]) for v in SAFE_PAIRS.values()} <= tails, fam.name
    # the lane widths the lengths were chosen for, and the units
    for n, c in SCAN5_C.items():
        assert scan5_c(n) == c and len(unit_slices(n)) == 1
    assert unit_slices(8193) == [(0, 4097), (4097, 8193)] and unit_slices(20000) == [(0, 6667), (6667, 13334), (13334, 20000)]
    assert {scan5_c(hi - lo) % 16 == 0 for n in FULL for lo, hi in unit_slices(n)} == {True, False}

    # byte 0 and byte 15 of a piece, for every context-sensitive kind, in each geometry; where pieces do not overlap, no other
    # piece covers the byte
    geometries = {"scan3": ("scan3", FULL), "scan5, C % 16 == 0": ("scan5-small", (1000, 8192)), "scan5, C % 16 != 0": ("scan5-small", (1100, 20000))}
    for name, (judge, lengths) in geometries.items():
        for kind in SENSITIVE:
            seen = set()
            for n in lengths:
                for c in unsafe_family(n, "ascii").cases:
                    if c.kind != kind:
                        continue
                    cov = covering(n, judge, c.p)
                    if name.endswith("!= 0"):
                        if n == 1100 or scan5_c(unit_slices(n)[cov[0][0]][1] - unit_slices(n)[cov[0][0]][0]) % 16:
                            seen |= {b for _, b in cov}
                    elif len(cov) == 1:
                        seen.add(cov[0][1])
            assert {0, 15} <= seen, (name, kind, sorted(seen))
    # ... and of k_fold_safe's blocks, which are aligned in memory
    for kind in SENSITIVE:
        seen = {(int(fam.off[c.doc]) + c.p) % 16 for n in FULL for fam in [unsafe_family(n, "ascii")] for c in fam.cases if c.kind == kind}
        assert seen == set(range(16)), (kind, sorted(seen))

    # the trips of a unit's job list: in the dense documents every piece is a job, 64 to a trip -- eight trips in a unit of
    # 8 192 bytes, seven in the units of a document of 20 000 (417 pieces for scan3, 432 overlapping ones for scan5: a list that
    # cannot hold 512 may still hold those)
    for judge in JUDGES[:3]:
        for n in (8192, 20000):
            trips = set()
            fam = unsafe_family(n, "dense")
            for c in fam.cases[::7]:
                if c.kind not in SENSITIVE:
                    continue
                lo, _ = fam.span(c.doc)
                ulo, uhi = next(u for u in unit_slices(n) if u[0] <= c.p < u[1])
                jobs = unit_jobs(fam.blob, judge, lo + ulo, uhi - ulo)
                assert (len(jobs) == 512 if n == 8192 else 384 < len(jobs) < 512), (judge, n, len(jobs))
                for j, rel in enumerate(jobs):
                    if rel <= c.p - ulo < rel + 16:
                        trips.add("first" if j // 64 == 0 else "last" if j // 64 == (len(jobs) - 1) // 64 else "middle")
            assert trips == {"first", "middle", "last"}, (judge, n, trips)

    # the rim: a lone lead as the last byte at every length modulo 16, a continuation byte as the first at every address
    for f in FILLERS:
        fam = rim_family(f)
        ends = {(int(fam.off[c.doc + 1]) - int(fam.off[c.doc])) % 16 for c in fam.cases if c.kind in RIM_END}
        starts = {int(fam.off[c.doc]) % 16 for c in fam.cases if c.kind in RIM_START}
        assert ends == set(range(16)) and starts == set(range(16)), (f, sorted(ends), sorted(starts))
        # across the border stands a pair that the rule accepts
        assert any(c.kind in RIM_END and doc_safe(bytes(fam.doc(c.doc)[-1:]) + bytes(fam.doc(c.doc + 1)[:1])) for c in fam.cases)

    # the model, as the code stands, agrees with the reference wherever it is asked; read wrongly, it does not
    asked = list(_model_cases())
    for judge in JUDGES:
        for fam, i, want in asked:
            lo, hi = fam.span(fam.cases[i].doc)
            assert model_verdict(fam.blob, lo, hi, judge) == want, (judge, fam.name, fam.cases[i])
    # (two documents in one batch: only there does k_fold_safe need k_fold_doc_edges)
    for f in FILLERS:
        fam, pairs = rim_pairs(f)
        assert len(pairs) >= 64
        for d in pairs:
            for judge in JUDGES:
                assert model_batch_verdict(fam.blob, fam.off[d:d + 3], judge), (judge, fam.name, d)
        d = pairs[0]
        assert not model_batch_verdict(fam.blob, fam.off[d:d + 3], "k_fold_safe", READINGS[-1])
        log[(READINGS[-1], "k_fold_safe")] = "%s: documents %d and %d in one batch" % (fam.name, d, d + 1)
    for reading in READINGS[:-1]:
        judges = JUDGES if reading in ("C3 80..9E accepted", "C3 97 refused") else JUDGES[:3]
        for judge in judges:
            caught = None
            for fam, i, want in asked:
                lo, hi = fam.span(fam.cases[i].doc)
                if model_verdict(fam.blob, lo, hi, judge, reading) != want:
                    caught = "%s: %s at %d" % (fam.name, fam.cases[i].kind, fam.cases[i].p)
                    break
            assert caught, (reading, judge, "no case notices")
            log[(reading, judge)] = caught

    # ... and where a unit's list has eight trips, a violation that the last one alone holds
    fam = unsafe_family(8192, "dense")
    for judge in JUDGES[:3]:
        at = [c for c in fam.cases if c.kind in SENSITIVE and c.p + len(SENSITIVE[c.kind]) == 8192]
        lo, hi = fam.span(at[0].doc)
        assert model_verdict(fam.blob, lo, hi, judge) and not model_verdict(fam.blob, lo, hi, judge, "the last trip dropped"), judge
        log[("the last trip dropped", judge)] += "; %s: %s at %d" % (fam.name, at[0].kind, at[0].p)

    bad, good = n_single_cases()
    assert 0.3 < bad / (bad + good) < 0.7, (bad, good)


def _model_cases():
    """(family, case index, reference's verdict) on which the model is run: the rim, the ASCII sweeps of 1 000 and 1 100 bytes,
    every fifth case of 20 000 bytes, and a handful of dense documents"""
    for f in FILLERS:
        fam = rim_family(f)
        for i in range(len(fam.cases)):
            yield fam, i, True
    for n, step in ((1000, 1), (1100, 1), (20000, 5)):
        for which in ("unsafe", "safe"):
            fam = family(which, n, "ascii")
            for i in range(0, len(fam.cases), step):
                yield fam, i, bool(fam.unsafe[i])
    for which in ("unsafe", "safe"):
        fam = family(which, 1000, "dense")
        for i in range(0, len(fam.cases), 5):
            yield fam, i, bool(fam.unsafe[i])
    fam = unsafe_family(8192, "dense")
    for i in range(0, len(fam.cases), 97):
        yield fam, i, True
