"""Inputs and references for the sweep of the UTF-8 kernels over every code point and every short byte sequence
(tests/test_utf8_sweep_host.py: the host twins and the mutants; tests/test_gpu_utf8_sweep.py: the kernels).  No tests in here.

The tables LOWER[cp] and WORD[cp] come from the host library (gft_to_lower over all scalar values at once, gft_debug_word_rune),
which tests/test_tolower_host.py and tests/test_words_host.py pin to Unicode 13.0.0 -- never from the interpreter's unicodedata.
Byte sequences are cut into runes by word_cases.decode_rune / decode_last_rune, plain Python that shares nothing with the
kernels' piece headers; valid code points are encoded by utf8_of(), arithmetic on numpy arrays.  The layouts are put together
by rows(): ragged columns laid side by side, row after row, with no Python loop over runes.

The check_* functions are the comparisons of the GPU module.  On a mismatch they name the first differing code point or byte
sequence in hex; the host module feeds them outputs of altered references (the mutants) and expects each to be noticed."""
import ctypes as C
import functools

import numpy as np

import word_cases as WC
from gofindthem_amd import _lib

N_CP = 0x110000
ERR = WC.RUNE_ERROR
B = bytes.fromhex("00417F808F909FA0BFC0C3E2F0FF")
N_SEQS, N_HIGH_SEQS, N_HIGH_VALID = 350208, 149216, 8544
L3_BYTES, L3_LOWERED = 1455360, 2915550
W_AB_CELLS, W_AB_KEPT = 2924288, 2568298
N_CASED, N_CHANGERS = 1393, 25
CUT_LEADS = [b"\xc3", b"\xe2\x82", b"\xf0\x9f\x98"]
TAIL = b"\xbf\xbf\xbf"
FFFD = b"\xef\xbf\xbd"
J_HEAD, J_TAIL = b'{"a":"', b'"}'
J_OK, J_TEXT = 0, 6                                  # (json_docs.OK, json_docs.TEXT)
J_ESCAPE_PADS, J_HIGH_PADS = (0, 52, 53, 54, 55, 56, 57), (0, 55, 56, 57)
TERM_LEN = np.array([1, 2, 3, 4, 2], np.uint32)      # pseudo terms of 1 to 4 bytes (cell C: a sequence is its own entry), and `ab`
TERM_AB = 4


# ---- arrays of bytes -----------------------------------------------------------------------------------------------------------
def utf8_of(cps):
    """the UTF-8 of an array of scalar values -> (bytes uint8, lengths int64)"""
    cp = np.asarray(cps, np.uint32)
    n = 1 + (cp >= 0x80).astype(np.int64) + (cp >= 0x800) + (cp >= 0x10000)
    m = np.zeros((cp.size, 4), np.uint8)
    cont = lambda x, shift: (0x80 | ((x >> shift) & 0x3F)).astype(np.uint8)   # noqa: E731
    k = n == 1
    m[k, 0] = cp[k]
    k = n == 2
    m[k, 0], m[k, 1] = 0xC0 | (cp[k] >> 6), cont(cp[k], 0)
    k = n == 3
    m[k, 0], m[k, 1], m[k, 2] = 0xE0 | (cp[k] >> 12), cont(cp[k], 6), cont(cp[k], 0)
    k = n == 4
    m[k, 0], m[k, 1], m[k, 2], m[k, 3] = 0xF0 | (cp[k] >> 18), cont(cp[k], 12), cont(cp[k], 6), cont(cp[k], 0)
    return m[np.arange(4)[None, :] < n[:, None]], n


def fixed(b, n):
    """the column that holds the bytes b in each of n rows"""
    return np.tile(np.frombuffer(bytes(b), np.uint8), n), np.full(n, len(b), np.int64)


def starts_of(lens):
    return np.cumsum(lens) - lens


def rows(*cols):
    """ragged columns (bytes, lengths [n]) side by side -> (blob, col_start int64 [n_cols, n]: where each cell begins, row_off [n + 1])"""
    lens = np.stack([c[1] for c in cols]).astype(np.int64)
    row_off = np.zeros(lens.shape[1] + 1, np.int64)
    row_off[1:] = np.cumsum(lens.sum(0))
    col_start = row_off[:-1] + (np.cumsum(lens, 0) - lens)
    blob = np.empty(int(row_off[-1]), np.uint8)
    for (data, ln), st in zip(cols, col_start):
        blob[np.repeat(st - starts_of(ln), ln) + np.arange(data.size)] = data
    return blob, col_start, row_off


def take(col, pick):
    """the rows `pick` of a ragged column"""
    data, lens = col
    ln = lens[pick]
    return data[np.repeat(starts_of(lens)[pick] - starts_of(ln), ln) + np.arange(int(ln.sum()))], ln


def cat(a, b):
    return np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])


def u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def hexs(b):
    return bytes(b).hex(" ")


def first_diff(got, want):
    """the first index at which two flat arrays differ (their common length, when one is a prefix of the other), or None"""
    got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
    if got.size == want.size and np.array_equal(got, want):
        return None
    n = min(got.size, want.size)
    d = np.flatnonzero(got[:n] != want[:n])
    return int(d[0]) if d.size else n


# ---- the tables ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scalars():
    """every scalar value from U+0080 up: 1 111 936 of them"""
    cp = np.arange(0x80, N_CP, dtype=np.uint32)
    return cp[(cp < 0xD800) | (cp > 0xDFFF)]


def host_lower(data):
    """gft_to_lower over one buffer -> the lowered bytes as an array"""
    L = _lib.load()
    src = np.ascontiguousarray(data, np.uint8).tobytes()
    out = np.zeros(3 * len(src) + 1, np.uint8)
    need = C.c_uint64(0)
    assert L.gft_to_lower(src, len(src), out.ctypes.data, out.size, C.byref(need)) == 0
    return out[:need.value].copy()


@functools.lru_cache(maxsize=None)
def tables():
    """(LOWER uint32 [0x110000], WORD bool [0x110000]) from the host library; the surrogates map to themselves and are no word runes"""
    L = _lib.load()
    cp = np.arange(N_CP, dtype=np.uint32)
    cp = cp[(cp < 0xD800) | (cp > 0xDFFF)]
    low = host_lower(utf8_of(cp)[0]).tobytes().decode("utf-8")
    assert len(low) == cp.size
    lower = np.arange(N_CP, dtype=np.uint32)
    lower[cp] = np.frombuffer(low.encode("utf-32-le"), "<u4")
    f = L.gft_debug_word_rune
    word = np.fromiter((f(c) for c in range(N_CP)), np.uint8, N_CP).astype(bool)
    lower.setflags(write=False)
    word.setflags(write=False)
    return lower, word


# ---- the byte sequences --------------------------------------------------------------------------------------------------------
def _product(*axes):
    g = np.meshgrid(*[np.asarray(list(a), np.uint8) for a in axes], indexing="ij")
    return np.stack([x.ravel() for x in g], 1)


def make_seqs(high):
    """SEQS (high False) or HIGH_SEQS (the same construction over the bytes >= 0x80) -> (bytes, lengths)"""
    every = range(0x80, 0x100) if high else range(0x100)
    b = [x for x in B if x >= 0x80] if high else list(B)
    groups = [_product(every), _product(range(0x80, 0x100), every), _product(range(0xC0, 0x100), every, b),
              _product(range(0xE0, 0x100), b, b, b)]
    return np.concatenate([g.ravel() for g in groups]), np.concatenate([np.full(len(g), g.shape[1], np.int64) for g in groups])


def as_list(col):
    """a ragged column (or blob, offsets) as a list of bytes objects"""
    data, lens = col
    raw, at = np.asarray(data, np.uint8).tobytes(), np.concatenate([[0], np.cumsum(lens)]).tolist()
    return [raw[a:b] for a, b in zip(at[:-1], at[1:])]


class Seqs:
    """a list of byte sequences of 1 to 4 bytes, each cut into Go's runes in plain Python: col (bytes, lengths); n_runes [n]; per
    rune (padded to 4 per sequence) cp (-1: one invalid byte), a (first byte), sl (bytes); first / last: the code point that
    DecodeRune / DecodeLastRune give for the sequence, -1 for RuneError; valid: every rune is one"""

    def __init__(self, col, decode=WC.decode_rune, decode_last=WC.decode_last_rune):
        self.col = col
        self.list = as_list(col)
        n = len(self.list)
        cp, a, sl = np.full((n, 4), -1, np.int64), np.zeros((n, 4), np.int64), np.zeros((n, 4), np.int64)
        first, last, n_runes = np.full(n, -1, np.int64), np.full(n, -1, np.int64), np.zeros(n, np.int64)
        for i, s in enumerate(self.list):
            at = k = 0
            while at < len(s):
                r, size = decode(s[at:])
                cp[i, k], a[i, k], sl[i, k] = (-1 if r == ERR and size == 1 else r), at, size
                at += size
                k += 1
            n_runes[i] = k
            first[i] = cp[i, 0]
            r, size = decode_last(s)
            last[i] = -1 if r == ERR and size == 1 else r
        self.cp, self.a, self.sl, self.first, self.last, self.n_runes = cp, a, sl, first, last, n_runes
        self.is_rune = np.arange(4)[None, :] < n_runes[:, None]
        self.valid = ((cp >= 0) | ~self.is_rune).all(1)

    def __len__(self):
        return len(self.list)

    def lowered(self, lower):
        """(column of the lowered sequences, b [n, 4]: first lowered byte of each rune, ll [n, 4]: its lowered bytes)"""
        low = np.where(self.cp < 0, ERR, lower[np.maximum(self.cp, 0)])
        data, ln = utf8_of(low[self.is_rune])
        ll = np.zeros(self.cp.shape, np.int64)
        ll[self.is_rune] = ln
        return (data, ll.sum(1)), np.cumsum(ll, 1) - ll, ll

    def label(self, i):
        return "sequence %s (index %d)" % (hexs(self.list[i]), i)


@functools.lru_cache(maxsize=None)
def seqs():
    return Seqs(make_seqs(False))


@functools.lru_cache(maxsize=None)
def high_seqs():
    return Seqs(make_seqs(True))


def cp_label(cp):
    return "U+%04X" % int(cp)


# ---- to_lower and map_spans_to_source ------------------------------------------------------------------------------------------------
class Batch:
    """a batch for gft_to_lower_device with its reference, and the runes to map back: blob, doc_off [n + 1]; want, want_off: the
    lowered batch; spans(): (span_off, start, len) of lowered spans and the (start, len) they must come back as; label_at(i): who
    owns byte i of `want`; label_doc(d); label_span(k)"""

    def __init__(self, name, blob, doc_off, want, want_off):
        self.name, self.blob, self.doc_off, self.want, self.want_off = name, blob, u64(doc_off), want, u64(want_off)
        self.n_docs = self.doc_off.size - 1

    def label_doc(self, d):
        return "document %d" % d

    def label_at(self, i):
        return self.label_doc(int(np.searchsorted(self.want_off, i, side="right")) - 1)


def l1(shifts=range(16), lower=None):
    """document s: s bytes `Z`, then every scalar value from U+0080 up -- every rune at every position of the 16-byte piece"""
    lower = tables()[0] if lower is None else lower
    shifts = list(shifts)
    cp = scalars()
    src, sl = utf8_of(cp)
    low, ll = utf8_of(lower[cp])
    blob = np.concatenate([x for s in shifts for x in (np.full(s, ord("Z"), np.uint8), src)])
    want = np.concatenate([x for s in shifts for x in (np.full(s, ord("z"), np.uint8), low)])
    off = np.concatenate([[0], np.cumsum([s + src.size for s in shifts])])
    woff = np.concatenate([[0], np.cumsum([s + low.size for s in shifts])])
    b = Batch("L1", blob, off, want, woff)
    b.shifts, b.cp, b.a, b.sl, b.b, b.ll = shifts, cp, starts_of(sl), sl, starts_of(ll), ll

    def label_at(i):
        d = int(np.searchsorted(b.want_off, i, side="right")) - 1
        rel = i - int(b.want_off[d]) - shifts[d]
        if rel < 0:
            return "the Z run of document %d" % d
        return "%s in document %d" % (cp_label(cp[int(np.searchsorted(b.b, rel, side="right")) - 1]), d)
    b.label_at = label_at
    b.label_doc = lambda d: "document %d (shift %d)" % (d, shifts[d])
    b.label_span = lambda k: "%s in document %d" % (cp_label(cp[k % cp.size]), k // (2 * cp.size))

    def spans():
        st = np.concatenate([x for s in shifts for x in (s + b.b, s + b.b + b.ll - 1)])
        ln = np.concatenate([x for s in shifts for x in (b.ll, np.ones(cp.size, np.int64))])
        w_st = np.concatenate([s + b.a for s in shifts for _ in (0, 1)])
        w_ln = np.concatenate([b.sl for s in shifts for _ in (0, 1)])
        return u64(np.arange(len(shifts) + 1) * 2 * cp.size), st, ln, w_st, w_ln
    b.spans = spans
    return b


def l2(lower=None):
    """every scalar value from U+0080 up as a document of its own: the neighbours' bytes would continue or lead each rune"""
    lower = tables()[0] if lower is None else lower
    cp = scalars()
    src, sl = utf8_of(cp)
    low, ll = utf8_of(lower[cp])
    b = Batch("L2", src, np.concatenate([[0], np.cumsum(sl)]), low, np.concatenate([[0], np.cumsum(ll)]))
    b.cp, b.sl, b.ll = cp, sl, ll
    b.label_doc = lambda d: "%s (document %d)" % (cp_label(cp[d]), d)
    b.label_span = lambda k: cp_label(cp[k // 2])

    def spans():
        st = np.stack([np.zeros(cp.size, np.int64), ll - 1], 1).ravel()
        ln = np.stack([ll, np.ones(cp.size, np.int64)], 1).ravel()
        return u64(np.arange(cp.size + 1) * 2), st, ln, np.zeros(2 * cp.size, np.int64), np.repeat(sl, 2)
    b.spans = spans
    return b


def l3(per_document, sq=None, lower=None, every=1):
    """the sequences of SEQS: as one document, b"Z" behind each; or each a document of its own with a document BF BF BF behind it.
    every: only each every-th sequence.  spans(): one span per lowered rune of the sequences, and the source runes' (start, len)"""
    lower = tables()[0] if lower is None else lower
    sq = seqs() if sq is None else sq
    pick = np.arange(0, len(sq), every)
    n = pick.size
    src_col = take(sq.col, pick)
    low_col, b_rel, ll = sq.lowered(lower)
    low_col = take(low_col, pick)
    b_rel, ll, a_rel, sl, is_rune = b_rel[pick], ll[pick], sq.a[pick], sq.sl[pick], sq.is_rune[pick]
    if per_document:
        blob, cs, row_off = rows(src_col, fixed(TAIL, n))
        want, wcs, wrow_off = rows(low_col, fixed(FFFD * 3, n))
        off = np.append(cs.T.ravel(), row_off[-1])
        woff = np.append(wcs.T.ravel(), wrow_off[-1])
        bt = Batch("L3 per document", blob, off, want, woff)
        bt.label_doc = lambda d: sq.label(int(pick[d // 2])) if d % 2 == 0 else "the document BF BF BF behind " + sq.label(int(pick[d // 2]))
        base_src = base_low = np.zeros(n, np.int64)
        counts = np.stack([sq.n_runes[pick], np.zeros(n, np.int64)], 1).ravel()
    else:
        blob, cs, row_off = rows(src_col, fixed(b"Z", n))
        want, wcs, wrow_off = rows(low_col, fixed(b"z", n))
        bt = Batch("L3 in one document", blob, [0, blob.size], want, [0, want.size])
        bt.label_at = lambda i: sq.label(int(pick[int(np.searchsorted(wcs[0], i, side="right")) - 1]))
        base_src, base_low = cs[0], wcs[0]
        counts = np.array([int(sq.n_runes[pick].sum())])
    owner = np.repeat(np.arange(n), sq.n_runes[pick])
    bt.label_span = lambda k: sq.label(int(pick[owner[k]]))

    def spans():
        so = np.concatenate([[0], np.cumsum(counts)])
        return (u64(so), (base_low[:, None] + b_rel)[is_rune], ll[is_rune], (base_src[:, None] + a_rel)[is_rune], sl[is_rune])
    bt.spans = spans
    return bt


def check_lower(batch, out, out_off, total, want=None, want_off=None):
    """what gft_to_lower_device (or a twin) gave for a batch against the reference: the total, every offset, every byte"""
    want = batch.want if want is None else want
    want_off = batch.want_off if want_off is None else want_off
    if out is not None:
        i = first_diff(np.asarray(out, np.uint8)[:min(int(total), want.size)], want)
        assert i is None, "%s: lowered byte %d differs: %s" % (batch.name, i, batch.label_at(min(i, want.size - 1)))
    d = first_diff(np.asarray(out_off, np.uint64), want_off)
    assert d is None, "%s: the lowered offset %d differs: %s" % (batch.name, d, batch.label_doc(max(d - 1, 0)))
    assert int(total) == want.size, "%s: total %d, not %d" % (batch.name, int(total), want.size)


def check_spans(batch, got_start, got_len, want_start, want_len):
    for got, want, what in ((got_start, want_start, "start"), (got_len, want_len, "length")):
        k = first_diff(np.asarray(got).astype(np.int64) & 0xFFFFFFFF, np.asarray(want, np.int64))
        assert k is None, "%s: the mapped %s of span %d differs: %s" % (batch.name, what, k, batch.label_span(k))


# ---- the word filter -------------------------------------------------------------------------------------------------------------
class Words:
    """the cells A = s + b"ab " (entry `ab`), B = b" ab" + s (entry `ab`) and C = b"a" + s + b"a" (entry s) for every scalar value from
    U+0080 up and every sequence of SEQS, as entries of a few large documents (per_document False) or one cell per document, a
    document ending in a cut lead in front of every A and a document BF BF BF behind every B.  The arrays are those of
    word_cases.Case: blob, doc_off, off, pos (first bytes), length, term, term_len; keep [n]: the rule of word_cases.kept with WORD"""

    def __init__(self, per_document, sq=None, word=None, last=None, big_docs=4):
        word = tables()[1] if word is None else word
        sq = seqs() if sq is None else sq
        cp = scalars()
        self.sq, self.cp, self.per_document = sq, cp, per_document
        s = cat(utf8_of(cp), sq.col)
        n = s[1].size
        self.n_sources = n
        is_word = lambda r: np.where(r < 0, False, word[np.maximum(r, 0)]) & (r != ERR)     # noqa: E731  (word_cases.is_word)
        fw = np.concatenate([word[cp], is_word(sq.first)])
        lw = np.concatenate([word[cp], is_word(sq.last if last is None else last)])
        # kept(): the occurrence's own first and last rune are `a`, `b` (word runes) in A and B, its neighbours `a` (a word rune) in C;
        # a space and a document's border are none
        self.keep = np.stack([~lw, ~fw, ~fw & ~lw], 1).ravel()
        f = lambda b: fixed(b, n)                                   # noqa: E731
        if per_document:
            lead = [np.frombuffer(x, np.uint8) for x in CUT_LEADS]
            which = np.arange(n) % 3
            cut = (np.concatenate([np.frombuffer(b"".join(CUT_LEADS), np.uint8)] * (n // 3) + lead[:n % 3]), np.array([1, 2, 3], np.int64)[which])
            blob, cs, row_off = rows(cut, s, f(b"ab "), f(b" ab"), s, f(TAIL), f(b"a"), s, f(b"a"))
            doc_off = np.append(cs[[0, 1, 3, 5, 6]].T.ravel(), row_off[-1])
            pos = np.stack([s[1], np.ones(n, np.int64), np.ones(n, np.int64)], 1).ravel()
            counts = np.tile(np.array([0, 1, 1, 0, 1], np.int64), n)
        else:
            blob, cs, row_off = rows(s, f(b"ab "), f(b" ab"), s, f(b"a"), s, f(b"a"))
            cut_rows = np.linspace(0, n, big_docs + 1).astype(np.int64)
            doc_off = row_off[cut_rows]
            doc_of_row = np.searchsorted(cut_rows, np.arange(n), side="right") - 1
            pos = (np.stack([cs[1], cs[2] + 1, cs[5]], 1) - doc_off[doc_of_row][:, None]).ravel()
            counts = 3 * np.diff(cut_rows)
        self.blob = np.concatenate([blob, np.full(64, ord("a"), np.uint8)])
        self.doc_off, self.n_docs = u64(doc_off), doc_off.size - 1
        self.off = u64(np.concatenate([[0], np.cumsum(counts)]))
        self.pos = pos.astype(np.uint32)
        self.length = np.stack([np.full(n, 2), np.full(n, 2), s[1]], 1).ravel().astype(np.uint32)
        self.term = np.stack([np.full(n, TERM_AB), np.full(n, TERM_AB), s[1] - 1], 1).ravel().astype(np.uint32)
        self.term_len, self.n = TERM_LEN, 3 * n
        self.name = "W, one cell per document" if per_document else "W, %d large documents" % big_docs
        self.entry_doc = np.repeat(np.arange(self.n_docs), counts)

    def pos_for(self, pos_end):
        return (self.pos + self.length - 1).astype(np.uint32) if pos_end else self.pos

    def reference(self, pos_end=False):
        """(out_off uint64 [n_docs + 1], pos, len, term uint32 [total])"""
        out_off = np.zeros(self.n_docs + 1, np.int64)
        out_off[1:] = np.cumsum(np.bincount(self.entry_doc[self.keep], minlength=self.n_docs))
        return u64(out_off), self.pos_for(pos_end)[self.keep], self.length[self.keep], self.term[self.keep]

    def label(self, entry):
        src, cell = divmod(int(entry), 3)
        who = cp_label(self.cp[src]) if src < self.cp.size else self.sq.label(src - self.cp.size)
        return "cell %s of %s" % ("ABC"[cell], who)


@functools.lru_cache(maxsize=None)
def words(per_document):
    return Words(per_document)


def check_words(w, total, out_off, pos, length, term, pos_end=False, reference=None):
    """what gft_filter_word_matches_device (or its twin) gave for a layout against the reference: out_off, pos, len and term.  The
    first kept entry that differs lies behind the last one that agreed: among the entries from there to the one expected, the
    culprit is in the first document whose offset differs and, if it was wrongly kept, has the position that came back"""
    w_off, w_pos, w_len, w_term = reference if reference is not None else w.reference(pos_end)
    got_off = np.asarray(out_off).view(np.uint64)[:w.n_docs + 1]
    n = min(int(total), w_pos.size)
    got = [np.asarray(a).view(np.uint32)[:n] for a in (pos, length, term)]
    ks = [first_diff(g, x[:n]) for g, x in zip(got, (w_pos, w_len, w_term))]
    d = first_diff(got_off, w_off)
    if d is None and int(total) == w_pos.size and all(k is None for k in ks):
        return
    kept = np.flatnonzero(w.keep)
    k = min([k for k in ks if k is not None] + [n])
    cand = np.arange(int(kept[k - 1]) + 1 if k else 0, int(kept[k]) + 1 if k < kept.size else w.n)
    if d is not None and int(w.off[max(d, 1)] - w.off[max(d, 1) - 1]) <= 3:      # (equal entries behind it can hide a shift from k)
        cand = np.arange(int(w.off[max(d, 1) - 1]), int(w.off[max(d, 1)]))
    elif k < n and (w.pos_for(pos_end)[cand] == got[0][k]).any():
        cand = cand[w.pos_for(pos_end)[cand] == got[0][k]]
    elif cand.size > 3:
        cand = cand[-1:]
    raise AssertionError("%s: total %d, expected %d; kept entry %d differs (first offset that differs: %s): %s" % (
        w.name, int(total), w_pos.size, k, d, ", ".join(w.label(e) for e in cand[:3])))


# ---- JSON ----------------------------------------------------------------------------------------------------------------------------
_HEX = (np.frombuffer(b"0123456789abcdef", np.uint8), np.frombuffer(b"0123456789ABCDEF", np.uint8))


class Json:
    """documents {"a":" + b"p" * pad + payload + "} for the schema ["a"]: blob, doc_off; status [n] and, for the documents that are
    OK, the text each must decode to (text, text_off); label(d)"""

    def __init__(self, name, pad, payload, ok, text, label):
        n = payload[1].size
        self.name, self.pad, self.n_docs, self.label = name, pad, n, label
        self.blob, cs, row_off = rows(fixed(J_HEAD, n), fixed(b"p" * pad, n), payload, fixed(J_TAIL, n))
        self.doc_off = u64(row_off)
        self.status = np.where(ok, J_OK, J_TEXT).astype(np.uint8)
        p = np.full(n, pad, np.int64)
        self.text = rows(fixed(b"p" * pad, n), (text[0], text[1]))[0][np.repeat(ok, p + text[1])]
        self.text_off = u64(np.concatenate([[0], np.cumsum((p + text[1])[ok])]))      # (one leaf per OK document)
        self.rec_off = u64(np.concatenate([[0], np.cumsum(ok)]))

    def docs(self):
        return as_list((self.blob, np.diff(self.doc_off.astype(np.int64))))


def json_escapes(pad, value_of=None):
    """every \\uXXXX, in lower-case and in upper-case hex, behind `pad` bytes: the escape starts at byte 6 + pad of the document"""
    v = np.repeat(np.arange(0x10000, dtype=np.int64), 2)
    case = np.tile(np.array([0, 1]), 0x10000)
    m = np.zeros((v.size, 6), np.uint8)
    m[:, 0], m[:, 1] = ord("\\"), ord("u")
    for k in range(4):
        digit = (v >> (12 - 4 * k)) & 15
        m[:, 2 + k] = np.where(case == 0, _HEX[0][digit], _HEX[1][digit])
    decoded = v if value_of is None else value_of(v)
    ok = (decoded < 0xD800) | (decoded > 0xDFFF)
    text = utf8_of(np.where(ok, decoded, 0x3F))
    return Json("J, \\u escapes at pad %d" % pad, pad, (m.ravel(), np.full(v.size, 6, np.int64)), ok, text,
                lambda d: "\\u%s" % bytes(m[d, 2:]).decode())


def json_high(pad, hs=None, valid=None):
    hs = high_seqs() if hs is None else hs
    return Json("J, high-byte sequences at pad %d" % pad, pad, hs.col, hs.valid if valid is None else valid, hs.col, hs.label)


def json_raw(part=0, parts=1):
    """the raw UTF-8 of every scalar value from U+0080 up; part k of `parts` equal runs of them"""
    cp = scalars()
    cp = cp[cp.size * part // parts:cp.size * (part + 1) // parts]
    col = utf8_of(cp)
    return Json("J, raw UTF-8, part %d of %d" % (part + 1, parts), 0, col, np.ones(cp.size, bool), col, lambda d: cp_label(cp[d]))


def check_json(j, status, rec_off, leaf_field, leaf_off, text, totals, reference=None):
    """the record form that the JSON walker gave for a layout against the expected statuses and texts (one leaf, field 0, per OK
    document)"""
    r = j if reference is None else reference
    d = first_diff(np.asarray(status, np.uint8), r.status)
    assert d is None, "%s: the status of document %d is %d, not %d: %s" % (j.name, d, int(np.asarray(status)[d]), int(r.status[d]), j.label(d))
    assert first_diff(np.asarray(rec_off).astype(np.uint64), r.rec_off) is None, j.name
    n_leaves, n_text = int(r.rec_off[-1]), int(r.text_off[-1])
    assert tuple(int(x) for x in totals) == (n_leaves, n_text), (j.name, totals, n_leaves, n_text)
    owner = np.flatnonzero(r.status == J_OK)
    assert not np.asarray(leaf_field)[:n_leaves].any(), j.name
    k = first_diff(np.asarray(leaf_off)[:n_leaves + 1].astype(np.uint64), r.text_off)
    assert k is None, "%s: the text offset of leaf %d differs: %s" % (j.name, k, j.label(owner[max(k - 1, 0)]))
    i = first_diff(np.asarray(text, np.uint8)[:n_text], r.text)
    assert i is None, "%s: text byte %d differs: %s" % (j.name, i, j.label(owner[int(np.searchsorted(r.text_off, i, side="right")) - 1]))


# ---- the finder ------------------------------------------------------------------------------------------------------------------
class FinderCase:
    """one document x<cp>y for each of the 1 393 cased code points (A to Z among them) and every 97th uncased one from U+0080 up; the
    keywords: the 1 384 distinct lower forms of the cased ones, and `x` once more, last.  hits(whole_words) -> bool [n_docs,
    n_keywords]: document i hits keyword j when LOWER[cp_i] is j's rune -- and, the documents being what they are, when j is `x` or
    `y`, which are lower forms themselves"""

    def __init__(self, lower=None, word=None):
        t = tables()
        lower, word = t[0] if lower is None else lower, t[1] if word is None else word
        cp = np.concatenate([np.arange(0x41, 0x5B, dtype=np.uint32), scalars()])
        cased = lower[cp] != cp
        self.cp = np.concatenate([cp[cased], cp[~cased][::97]])
        self.n_cased = int(cased.sum())
        self.runes = np.append(np.unique(lower[cp[cased]]), np.uint32(ord("x")))
        n = self.cp.size
        self.blob, _, row_off = rows(fixed(b"x", n), utf8_of(self.cp), fixed(b"y", n))
        self.doc_off = u64(row_off)
        self.keywords = [chr(int(r)) for r in self.runes]
        self.low, self.word = lower[self.cp], word

    def hits(self, whole_words=False):
        mid = self.low[:, None] == self.runes[None, :]
        edge = np.isin(self.runes, [ord("x"), ord("y")])[None, :]
        if not whole_words:
            return mid | edge
        # `x` and `y` are word runes: the rune between them is a whole word only when it is none, and lets them be whole words then
        return (mid & ~self.word[self.runes][None, :]) | (edge & ~self.word[self.low][:, None])

    def label(self, d):
        return cp_label(self.cp[d])


def check_hits(f, got, whole_words=False, want=None):
    want = f.hits(whole_words) if want is None else want
    k = first_diff(got, want)
    if k is not None:
        d, j = divmod(k, want.shape[1])
        raise AssertionError("the finder, whole words %s: document %s and keyword %r: hit %s, expected %s" % (
            whole_words, f.label(d), f.keywords[j], bool(np.asarray(got)[d, j]), bool(want[d, j])))


def unpack_rows(bitmap, n_cols):
    """uint32 rows [n, ceil(n_cols / 32)] -> bool [n, n_cols]"""
    bits = np.unpackbits(np.ascontiguousarray(bitmap).view(np.uint8), axis=1, bitorder="little")
    return bits[:, :n_cols].astype(bool)


# ---- that the sweep sweeps -------------------------------------------------------------------------------------------------------
def assert_not_vacuous():
    lower, word = tables()
    cp = scalars()
    every = np.zeros(N_CP, bool)
    every[cp] = True
    b1, b2 = l1(), l2()
    w = words(False)
    j = json_raw()
    for what, seen in (("L1", b1.cp), ("L2", b2.cp), ("W", w.cp), ("J", cp[j.status == J_OK])):
        got = np.zeros(N_CP, bool)
        got[seen] = True
        assert np.array_equal(got, every), what
    assert len(b1.shifts) == 16 and b1.want.size == sum(b1.shifts) + 16 * utf8_of(lower[cp])[0].size
    # the reference changes 1 393 code points, A to Z among them: each document of L1 holds the other 1 367, and its run of `Z`
    changed = lower[b1.cp] != b1.cp
    assert int((lower != np.arange(N_CP)).sum()) == N_CASED and int(changed.sum()) == N_CASED - 26
    assert int((b1.sl != b1.ll).sum()) == N_CHANGERS and int((b1.sl != b1.ll)[changed].sum()) == N_CHANGERS
    for per_document in (False, True):
        keep = words(per_document).keep
        assert int((~keep).sum()) > 300000 and int(keep.sum()) > 2000000
    for pad in J_ESCAPE_PADS:
        s = json_escapes(pad).status
        assert (s == J_OK).any() and int((s == J_TEXT).sum()) == 2 * 2048
    for pad in J_HIGH_PADS:
        s = json_high(pad).status
        assert int((s == J_OK).sum()) == N_HIGH_VALID and (s == J_TEXT).any()
