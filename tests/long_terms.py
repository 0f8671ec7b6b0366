"""Keywords of 301 to 7 424 bytes (test infrastructure: no GPU, no torch, nothing of the product): seeded builders of
(dictionary, documents) families around the longest keyword gft_build accepts (kTextBuf - 1024 = 7 424 bytes, plan_scan in
csrc/table_set.cpp), a brute-force match list in plain Python, and the solver scenario in which the answer of an INORD group
depends on a 7 424-byte match being found in a work unit thirteen places behind the one that already gave a candidate.
Shared by test_long_terms_host.py (which shows on the CPU that the families are what they claim and that the oracle agrees
with the brute force at these lengths), test_scan3_tables.py / test_scan5_tables.py (host emulations of the table walks) and
test_gpu_long_terms.py (the kernels against the oracle).

Every dictionary holds ONE keyword length L as its maximum -- the kernels' warm-up, look-back and position bias are functions
of max_term_len -- next to keywords of one to four bytes: the short-term tables stay in play, and with three of the eight
letters of the text as keywords the match density (> 0.25 per byte) makes `learn` (csrc/batch_verdict.cpp) shrink the work
units of the suffix-window kernels to 512 bytes for the second call on the same engine."""
import functools

import numpy as np

from oracle.pyoracle import Oracle, POS_END, POS_START, pack_strings

LENGTHS = (301, 512, 513, 1024, 4096, 7423, 7424)
MAX_LEN = 7424                                  # kTextBuf - 1024
POS_MODES = (POS_START, POS_END)
FAMILIES = ("planted", "periodic", "near_misses", "shared_suffix", "folded")
FOLDED = ("folded",)                            # the families that are scanned with fold=True
DOC_MAX = 40_000                                # no document is longer
TEXT_BUF = 8448                                 # kTextBuf: a wave's LDS text buffer, the DFA kernel's unit + warm-up
UNIT_SIZES = (512, 1025, 8192)                  # learnt minimum of scan5; kTextBuf - (7 424 - 1) of the DFA kernel; kScan2UnitMax
ALPHA = b"abcdefgh"
SHORT = [b"a", b"b", b"c", b"de", b"fgh", b"hgfe"]
E_ACUTE = "é".encode("utf-8")


def unit_slice(n, unit_max):
    """bytes per work unit of a document of n bytes (unit_slice of gft_kernels.hpp: k_unit_fill, and the host's unit table in gft_pipeline.cpp): equal slices"""
    k = 1 if n <= unit_max else (n + unit_max - 1) // unit_max
    return (n + k - 1) // k if n else 0


def _rng(family, L, salt=0):
    return np.random.default_rng([FAMILIES.index(family), L, salt])


def _noise(rng, n, letters=False):
    """n bytes over a-h; letters: a few of them replaced by whole two-byte letters"""
    buf = bytearray(ALPHA[int(i)] for i in rng.integers(0, len(ALPHA), n))
    if letters and n >= 2:
        last = -2
        for at in sorted(int(i) for i in rng.integers(0, n - 1, n // 40 + 1)):
            if at >= last + 2:
                buf[at:at + 2] = E_ACUTE
                last = at
    return bytes(buf)


def _other(byte):
    """another letter of the alphabet"""
    return ALPHA[(ALPHA.index(byte) + 1) % len(ALPHA)]


def _changed(kw, at):
    return kw[:at] + bytes([_other(kw[at])]) + kw[at + 1:]


# ---- planted -----------------------------------------------------------------------------------------------------------
SPAN_UNIT = unit_slice(DOC_MAX, 512)            # 507: the slices of a 40 000-byte document at 512-byte units
SPANS = (1, 7, 14)


@functools.lru_cache(maxsize=None)
def planted_layout(L, letters=False, family="planted"):
    """-> (terms, documents, layout); layout = [(document, start, keyword, what)]: where each long keyword was written.

    The long keyword K (L bytes) starts at byte 0 of the batch's first document, is a whole document, and ends on the last
    byte of the last document (the blob's last byte).  In documents of 40 000 bytes it ends at bytes per - 2, per - 1, 0 and 1
    of a unit, for per = the slice such a document gets at unit sizes of 512, 1 025 and 8 192 bytes (507, 1 000, 8 000) -- its
    last byte is the last but one and the last of a unit and the first and second of the next.  Keywords of j * 507 + 1 bytes
    (j = 1, 7, 14, where shorter than L) start on the last byte of a 507-byte unit and end j units later.  At 7 423 and 7 424
    bytes a document of ten times kTextBuf - (L - 1) bytes is cut by the DFA kernel into units of exactly that size (1 026,
    1 025), which with their warm-up of L - 1 bytes fill its text buffer to the last byte; K ends on the ninth unit's last byte."""
    rng = _rng(family, L, int(letters))
    K = _noise(rng, L)
    spans = [(j, _noise(rng, j * SPAN_UNIT + 1)) for j in SPANS if j * SPAN_UNIT + 1 < L]
    terms = SHORT + [K] + [kw for _, kw in spans]
    targets = []
    for u in UNIT_SIZES:
        per = unit_slice(DOC_MAX, u)
        for r in (per - 2, per - 1, 0, 1):
            targets.append((K, len(K) - 1, per, r, "ends at byte %d of a %d-byte unit" % (r, per)))
    for j, kw in spans:
        targets.append((kw, 0, SPAN_UNIT, SPAN_UNIT - 1, "starts on a unit's last byte, ends %d units later" % j))
    big, cursor = [[]], 0
    for kw, anchor, per, r, what in targets:                 # first fit: byte (start + anchor) % per == r
        while True:
            s = cursor + (r - (cursor + anchor)) % per
            if s + len(kw) <= DOC_MAX:
                break
            assert cursor, "a keyword does not fit a document"
            big.append([])
            cursor = 0
        big[-1].append((s, kw, what))
        cursor = s + len(kw)
    docs, layout = [], []

    def add(parts, what=None):
        """parts: bytes (filler, written as is) or (keyword, what)"""
        at, out = 0, []
        for p in parts:
            if isinstance(p, tuple):
                layout.append((len(docs), at, p[0], p[1]))
                p = p[0]
            out.append(p)
            at += len(p)
        docs.append(b"".join(out))

    add([(K, "starts at byte 0 of the first document"), _noise(rng, 200, letters)])
    add([])
    for placements in big:
        parts, at = [], 0
        for s, kw, what in placements:
            parts += [_noise(rng, s - at, letters), (kw, what)]
            at = s + len(kw)
        add(parts + [_noise(rng, DOC_MAX - at, letters)])
    u = TEXT_BUF - (L - 1)                                   # the DFA kernel's unit size under this dictionary
    if 10 * u <= DOC_MAX:                                    # ten slices of exactly that size: unit + warm-up fill the buffer
        add([_noise(rng, 9 * u - L, letters), (K, "ends on the last byte of a unit that fills kTextBuf with its warm-up"), _noise(rng, u, letters)])
    add([(K, "is the whole document")])
    add([_noise(rng, 200, letters), (K, "ends on the blob's last byte")])
    assert all(len(d) <= DOC_MAX for d in docs) and len(big) <= 3
    return terms, docs, layout


def planted(L, letters=False):
    return planted_layout(L, letters)[:2]


def folded(L):
    """`planted` with half of the letters in upper case, for a scan with fold=True (the keywords stay lower-case)"""
    terms, docs, _ = planted_layout(L, False, "folded")
    rng = _rng("folded", L, 9)
    out = []
    for d in docs:
        up = rng.integers(0, 2, len(d)).astype(bool)
        a = np.frombuffer(d, dtype=np.uint8).copy()
        a[up] -= 32                                          # (every byte is one of a-h)
        out.append(a.tobytes())
    assert b"".join(out).lower() == b"".join(docs)
    return terms, out


# ---- periodic ----------------------------------------------------------------------------------------------------------
PERIODIC_EXTRA = 600              # occurrences of the long keyword per run: more than two fifos' worth (256 entries) in a row


def periodic(L):
    """keywords ("ab" * k)[:L] and "a" * L in runs of "ab" / "a" a little longer than L: long matches that overlap end at every
    (second) position, next to short ones at every position -- more than a 256-entry fifo holds in every unit of 512 bytes"""
    ab, aa = (b"ab" * (L // 2 + 1))[:L], b"a" * L
    terms = [b"a", b"ab", b"ba", b"aba", b"abab", ab, aa]
    n_ab = (L + 2 * PERIODIC_EXTRA) // 2
    docs = [b"a" * (L + PERIODIC_EXTRA), b"ab" * n_ab, b"", b"h" * 37 + b"a" * (L + PERIODIC_EXTRA) + b"h", b"ba" * n_ab + b"b"]
    return terms, docs


# ---- near misses -------------------------------------------------------------------------------------------------------
SPLITS = (1, 4, 25, "half", "all but one")


def near_misses(L):
    """the long keyword with one byte wrong, with its first byte missing at the very start of the blob, and cut in two by a
    document border: it occurs nowhere.  (The short keywords do.)"""
    rng = _rng("near_misses", L)
    K = _noise(rng, L)
    terms = SHORT + [K]
    docs = [K[1:] + _noise(rng, 100)]                        # nothing at all lies in front of this one
    for at in (0, L - 1, L // 2):
        docs.append(_noise(rng, 150) + _changed(K, at) + _noise(rng, 150))
    for j in SPLITS:
        j = {"half": L // 2, "all but one": L - 1}.get(j, j)
        docs.append(_noise(rng, 100) + K[:L - j])            # document d ends with the first L - j bytes ...
        docs.append(K[L - j:] + _noise(rng, 100))            # ... document d + 1 starts with the other j
    docs.append(b"")
    docs.append(K[:L - 1])                                   # the blob ends one byte short of a match
    return terms, docs


# ---- shared suffix -----------------------------------------------------------------------------------------------------
def shared_suffix(L):
    """long keywords that end with the same 32 bytes S (one bucket of the suffix-window tables; a slot holds 24 bytes inline,
    the rest is compared in term_blob).  K2, K3 and K7 are proper suffixes of K1 and S is one of all: one end position reports
    up to five lengths through out_link."""
    rng = _rng("shared_suffix", L)
    S = _noise(rng, 32)
    K1 = _noise(rng, L - 32) + S
    K2 = K1[1:]
    K3 = K1[-max(40, L // 2):]
    K7 = K1[-33:]
    body = _noise(rng, L - 33)
    K4 = body + bytes([_other(K1[-33])]) + S                 # (K7 does not end here)
    n5 = max(48, L // 3)
    K5 = _noise(rng, n5 - 32) + S
    terms = SHORT + [K1, K2, K3, K4, K5, S, K7]
    docs = [_noise(rng, 120) + K1 + _noise(rng, 80),
            _noise(rng, 90) + K4,
            K2 + _noise(rng, 50),                            # K1 without its first byte at a document's start
            _noise(rng, 60) + _changed(K1, 0) + _noise(rng, 60),
            _noise(rng, 70) + K5 + _noise(rng, 70),
            S,
            b"",
            _noise(rng, 40) + _changed(K1[-len(K3) - 1:], 0) + _noise(rng, 10),      # K3 behind a byte that is not K1's
            K1 + K4 + K5 + K1]
    return terms, docs


BUILDERS = {"planted": planted, "periodic": periodic, "near_misses": near_misses, "shared_suffix": shared_suffix, "folded": folded}


def family(name, L):
    """-> (terms, documents, fold)"""
    terms, docs = BUILDERS[name](L)
    return terms, docs, name in FOLDED


# ---- references --------------------------------------------------------------------------------------------------------
def brute_force(terms, docs, pos_mode, fold=False):
    """every occurrence of every keyword by bytes.find, per document in the oracle's canonical order: by the offset of the
    match's last byte, longest first; term ids count the sorted dictionary; positions are the first byte (POS_START) or the
    last (POS_END).  No automaton."""
    dictionary = sorted({bytes(t) for t in terms})
    moff, tid, pos = [0], [], []
    for d in docs:
        text = d.lower() if fold else d                      # (bytes.lower: ASCII letters only, as GFT_FOLD_ASCII)
        hits = []
        for i, t in enumerate(dictionary):
            at = text.find(t) if t else -1
            while at >= 0:
                end = at + len(t) - 1
                hits.append((end, -len(t), i, at if pos_mode == POS_START else end))
                at = text.find(t, at + 1)
        hits.sort()
        tid += [h[2] for h in hits]
        pos += [h[3] for h in hits]
        moff.append(len(tid))
    return np.asarray(moff, np.uint64), np.asarray(tid, np.uint32), np.asarray(pos, np.uint32)


@functools.lru_cache(maxsize=None)
def expected(name, L, pos_mode):
    """the oracle's CSR of a family (computed once per session; treat as read-only)"""
    terms, docs, fold = family(name, L)
    blob, off = pack_strings(docs)
    got = Oracle(terms, pos_mode).scan(blob, off, fold=fold)
    for a in got:
        a.setflags(write=False)
    return got


# ---- the solver scenario -----------------------------------------------------------------------------------------------
X, S_, Y = b"x", b"s", b"yw"                    # letters that the filler does not have
SOLVER_DENSE = [b"a", b"b", b"c"]
X_AT, L_AT, Y_IN, S_IN, Y_LATE, S_LATE = 10, 11, 300, 600, 8000, 9000
SOLVER_DOC = 20_000                             # 40 units of 500 bytes at 512-byte units, 3 at 8 192, 20 at 1 025


@functools.lru_cache(maxsize=None)
def solver_case():
    """-> dict(terms, L, M, docs, names, exprs).  L (7 424 bytes) and M (513 bytes) are written at byte 11, behind `x` at byte 10;
    both hold `y` at document byte 300, L also holds `s` at document byte 600 (behind M, `s` stands there in the filler).  So in
    start-position mode "the first L-or-s behind x" is 11 where the long keyword is found and 600 where it is not, and a `y` at
    300 and nowhere else answers the group only in the first case; the match of L ENDS at byte 7 434, thirteen 500-byte units
    behind the unit that holds `s`.  Documents: a / m = L / M intact, `y` at 300 only; *_late = one more `y` at 8 000;
    *_broken = the long keyword's last byte changed (it does not occur; the bytes of `y` and `s` stay)."""
    rng = np.random.default_rng(7424)

    def with_marks(n, marks):
        b = bytearray(_noise(rng, n))
        for at, kw in marks:
            b[at:at + len(kw)] = kw
        return bytes(b)
    L = with_marks(MAX_LEN, [(Y_IN - L_AT, Y), (S_IN - L_AT, S_)])
    M = with_marks(513, [(Y_IN - L_AT, Y)])

    def doc(n, long_kw, y_late, broken=False, extra=()):
        body = _changed(long_kw, len(long_kw) - 1) if broken else long_kw
        marks = [(X_AT, X), (L_AT, body), (S_LATE, S_)] + list(extra)
        if len(long_kw) < S_IN:
            marks.append((S_IN, S_))
        if y_late:
            marks.append((Y_LATE, Y))
        return with_marks(n, [m for m in marks if m[0] + len(m[1]) <= n])
    docs, names = [], []
    for name, kw in (("a", L), ("m", M)):
        for suffix, kwargs in (("", {}), ("_late", dict(y_late=True)), ("_broken", dict(broken=True)),
                               ("_broken_late", dict(broken=True, y_late=True))):
            docs.append(doc(SOLVER_DOC, kw, kwargs.get("y_late", False), kwargs.get("broken", False)))
            names.append(name + suffix)
    docs.append(doc(30_000, L, True)); names.append("a_30000")
    docs.append(doc(L_AT + MAX_LEN, L, False)); names.append("a_tight")          # L ends on the document's last byte
    terms = SOLVER_DENSE + [X, S_, Y, L, M]

    def q(t):
        return '"%s"' % t.decode("ascii")
    groups = []
    for kw in (L, M):
        groups += ['inord(%s and (%s or %s) and %s)' % (q(X), q(kw), q(S_), q(Y)),
                   'inord(%s and %s and %s)' % (q(X), q(kw), q(Y)),
                   'inord(%s and %s)' % (q(S_), q(kw)),
                   'inord(%s and %s)' % (q(kw), q(Y))]
    exprs = groups + ["not (%s)" % g for g in groups]
    return dict(terms=terms, L=L, M=M, docs=docs, names=names, exprs=exprs, n_groups=len(groups))


def solver_short_docs():
    """documents of fewer than 8 units at every unit size (below 4 096 bytes), M and the short keywords only, and empty ones"""
    c = solver_case()
    rng = np.random.default_rng(513)
    M = c["M"]
    out = [b"", X + M + Y, X + b"ab" + S_ + b"ab" + Y, Y + M + X, b"",
           _noise(rng, 9) + X + M + _noise(rng, 900) + S_ + _noise(rng, 100) + Y + _noise(rng, 200),
           _noise(rng, 9) + X + _changed(M, 512) + _noise(rng, 40) + S_ + _noise(rng, 2000),
           S_ + M, M, _noise(rng, 3000), X + S_ + Y]
    assert all(len(d) < 4096 for d in out)
    return out
