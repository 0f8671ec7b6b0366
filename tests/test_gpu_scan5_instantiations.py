"""k_scan5 is compiled once per launch constant: with positions (CSR callers, INORD groups) and without them (presence only).
Through the C ABI against the oracle, at the smallest shapes where one instantiation could differ from the other:

  * one engine that alternates presence-only and position launches over the same 64 documents -- the direct short-term table,
    the group-indexed one of a large alphabet, and a dictionary forced onto the global fingerprint table;
  * a unit of a few hundred bytes whose matches outgrow the fifo (the second walk, straight to the pool);
  * matches that end within the first 24 bytes and the last 4 bytes of the blob (the guarded text loads);
  * zero-length documents between non-empty ones.

Every bitmap and every CSR equals the oracle's; the pool entries of a presence-only launch equal the model of
tests/presence_once.py (every match where the short terms come from the group-indexed tables, which emit every occurrence),
those of a launch with positions the number of matches."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before libgft.so is loaded: both must share ONE HIP runtime, the one torch brings along)

import presence_once as po
from helpers import assert_csr_equal, docs, scan_plan, tree_to_program
from oracle import dsl_ref
from oracle.pyoracle import Oracle

pytestmark = pytest.mark.gpu

SLACK = 64                          # readable bytes behind the blob; they spell terms, which no launch may report


def _programs(eng, exprs):
    def slot_of(lit):
        t = eng.term_id(lit)
        assert t >= 0
        return t
    return [tree_to_program(dsl_ref.parse(x, True)[0], slot_of) for x in exprs]


class Harness:
    """one engine over `terms`; `plain` = expressions without an INORD group (presence-only launches), `inord` = the same with
    one (positions); once = the once-per-unit rule of short_trip holds (direct short-term table)"""

    def __init__(self, terms, plain, inord, once, slack=b""):
        from gofindthem_amd import _lib
        from gofindthem_amd.engine import Engine
        self.L = _lib.load()
        self.eng = Engine()
        self.eng.build(terms)
        assert self.L.gft_scan_kernel(self.eng._h).decode() == "scan5"
        self.terms, self.once = terms, once
        self.exprs = {"plain": plain, "inord": inord}
        self.oracle = {k: Oracle(terms) for k in self.exprs}
        for k, ex in self.exprs.items():
            self.oracle[k].set_expressions(ex, True)
        self.scan_oracle = Oracle(terms)
        self.model = po.Model(terms)
        self.slack = (slack * (SLACK // max(len(slack), 1) + 1))[:SLACK] if slack else bytes(SLACK)
        self.mode = None
        self.hip = C.CDLL("libamdhip64.so")

    def close(self):
        self.eng.close()

    def unit_max(self):
        um = C.c_uint32(0)
        assert self.L.gft_debug_learned_unit(self.eng._h, C.byref(um), None) == 0
        return um.value

    def entries(self):
        n = C.c_uint64(0)
        assert self.L.gft_debug_pool_entries(self.eng._h, C.byref(n)) == 0
        return int(n.value)

    def device(self, blob, off):
        t = torch.from_numpy(np.concatenate([blob, np.frombuffer(self.slack, np.uint8)])).cuda()
        o = torch.from_numpy(off.astype(np.int64)).cuda()
        return t, o

    def process(self, mode, blob, off, fold=False):
        """gft_process_device under the expressions of `mode`: bitmap and pool entries against the oracle and the model"""
        if mode != self.mode:
            self.eng.set_programs(_programs(self.eng, self.exprs[mode]))
            self.mode = mode
        unit_max = self.unit_max()
        t, o = self.device(blob, off)
        n = len(off) - 1
        bm = torch.zeros((n, (self.eng.n_exprs + 31) // 32), dtype=torch.int32, device="cuda")
        self.eng.process_device(t.data_ptr(), o.data_ptr(), n, bm.data_ptr(), fold=fold)
        torch.cuda.synchronize()
        got = bm.cpu().numpy().view(np.uint32)
        want = self.oracle[mode].process(blob, off, fold=fold)
        assert np.array_equal(got, want), (mode, np.argwhere(got != want)[:4].tolist())
        once, matches = self.model.entries(blob, off, unit_max, fold)
        print("%s unit_max %d: entries %d, model %d, matches %d" % (mode, unit_max, self.entries(), once, matches))
        assert self.entries() == (once if mode == "plain" and self.once else matches), mode
        return self.entries(), matches

    def csr(self, blob, off, fold=False):
        """gft_scan_device (positions): the CSR is the oracle's entry for entry, the pool holds every match"""
        want = self.scan_oracle.scan(blob, off, fold=fold)
        t, o = self.device(blob, off)
        n = len(off) - 1
        m = self.eng.scan_device(t.data_ptr(), o.data_ptr(), n, fold=fold)
        nm = int(m.n_matches)
        assert nm == want[1].size == self.entries()
        mo = np.zeros(n + 1, np.uint64)
        ti, ps = np.zeros(nm, np.uint32), np.zeros(nm, np.uint32)
        for dst, src, nbytes in ((mo, m.match_off, 8 * (n + 1)), (ti, m.term_id, 4 * nm), (ps, m.pos, 4 * nm)):
            if nbytes:
                assert self.hip.hipMemcpy(C.c_void_p(dst.ctypes.data), C.c_void_p(src), C.c_size_t(nbytes), C.c_int(2)) == 0
        assert_csr_equal((mo, ti, ps), want)
        return nm


# ---- the three dictionaries of the alternating launches -----------------------------------------------------------------
LENS = [0, 1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 33, 63, 64, 65, 100, 127, 128, 129, 200, 255, 256, 257, 300, 400, 500, 511, 512]


def _texts(rng, alphabet, terms, n_docs=64):
    """n_docs documents of at most 512 bytes: random text over `alphabet` with whole terms planted"""
    out = []
    for d in range(n_docs):
        n = LENS[d % len(LENS)] if d < 2 * len(LENS) else int(rng.integers(0, 513))
        body = bytearray(alphabet[i] for i in rng.integers(0, len(alphabet), n))
        for _ in range(n // 24):
            t = terms[int(rng.integers(len(terms)))]
            if len(t) <= n:
                at = int(rng.integers(0, n - len(t) + 1))
                body[at:at + len(t)] = t
        out.append(bytes(body))
    return out


def _direct():
    rng = np.random.default_rng(3)
    texts = _texts(rng, b"abcdefghx", po.TERMS)
    return Harness(po.TERMS, po.expressions(False), po.expressions(True), once=True, slack=b"abcdefgh"), texts


LARGE_ALPHABET = b"abcdefghijklmnopqrstuvwxyz0123456789 .-_"      # 40 byte classes: beyond the direct short-term table's 32


def _large_alphabet_terms():
    rng = np.random.default_rng(9)
    a = LARGE_ALPHABET
    terms = {bytes([b]) for b in a[::7]} | {a[i:i + 2] for i in range(0, 38, 5)} | {a[i:i + 3] for i in range(1, 37, 6)}
    for _ in range(90):
        terms.add(bytes(a[i] for i in rng.integers(0, len(a), int(rng.integers(4, 12)))))
    terms |= {a[i:i + 4] for i in range(0, 36, 3)}              # every byte of the alphabet is in some term
    return sorted(terms)


def _exprs_of(terms, inord):
    t = [po.lit(x) for x in terms]
    ex = t[:40] + ["not " + x for x in t[:6]] + ["%s and %s" % (t[i], t[i + 1]) for i in range(0, 20, 2)] + ["%s or %s" % (t[i], t[-1 - i]) for i in range(10)]
    if inord:
        ex.append("inord(%s and %s)" % (t[0], t[1]))
    return ex


def _sg():
    terms = _large_alphabet_terms()
    assert len({b for t in terms for b in t}) > 32 and min(len(t) for t in terms) == 1
    rng = np.random.default_rng(4)
    return Harness(terms, _exprs_of(terms, False), _exprs_of(terms, True), once=False, slack=LARGE_ALPHABET), _texts(rng, LARGE_ALPHABET, terms)


def _fpt_global():
    rng = np.random.default_rng(5)
    a = b"abcdefgh"
    terms = sorted({bytes(a[i] for i in rng.integers(0, 8, int(rng.integers(1, 10)))) for _ in range(300)})
    return Harness(terms, _exprs_of(terms, False), _exprs_of(terms, True), once=True, slack=a), _texts(rng, a, terms)


@pytest.mark.parametrize("which", ["direct", "large_alphabet", "fpt_global"])
def test_alternating_launches(which, monkeypatch):
    """presence, CSR, presence, INORD, presence, CSR on ONE engine and the same 64 documents: every launch picks its own
    instantiation and leaves nothing behind for the next"""
    if which == "fpt_global":
        monkeypatch.setenv("GFT_SCAN_FPT_GLOBAL", "1")       # (read when the tables are built)
    h, texts = {"direct": _direct, "large_alphabet": _sg, "fpt_global": _fpt_global}[which]()
    try:
        assert len(texts) == 64 and max(len(t) for t in texts) <= 512
        blob, off = docs(texts)
        total = 0
        for step in ("plain", "csr", "plain", "inord", "plain", "csr", "inord", "plain"):
            if step == "csr":
                total += h.csr(blob, off)
            else:
                entries, matches = h.process(step, blob, off)
                total += matches
                if step == "plain" and h.once:
                    assert entries < matches                 # (the once-per-unit rule did something)
        assert total > 8 * 64
    finally:
        h.close()


# ---- a unit that outgrows the fifo ---------------------------------------------------------------------------------------
OVERFLOW_TERMS = [b"b", b"ab", b"abab", b"babab", b"ababab", b"bababab", b"abababab", b"aabab", b"bbabab"]


def test_fifo_overflow_takes_the_direct_walk_in_both_instantiations():
    """one document of 400 bytes of "ab": every position ends a short term and, from the eighth byte on, five long terms that
    share the suffix "abab" (one bucket with several entries) -- far more matches than the fifo holds, so the unit is walked
    a second time with the appends going to the pool (terms only on the presence-only launch)"""
    fifo_cap = scan_plan(OVERFLOW_TERMS)[1]["fifo_cap"]
    plain = [po.lit(t) for t in OVERFLOW_TERMS] + ['"b" and not "aabab"', '"abab" or "bbabab"']
    h = Harness(OVERFLOW_TERMS, plain, plain + ['inord("ab" and "babab")'], once=True, slack=b"ab")
    try:
        doc = b"ab" * 200
        quiet = po.fill(40)
        for texts in ([doc], [quiet, doc, b"", doc[:399], quiet]):
            blob, off = docs(texts)
            for step in ("plain", "inord", "plain"):
                entries, matches = h.process(step, blob, off)
                assert matches > 2 * fifo_cap
                if step == "plain":
                    assert fifo_cap < entries < matches
            assert h.csr(blob, off) > 2 * fifo_cap
    finally:
        h.close()


# ---- the borders of the blob ----------------------------------------------------------------------------------------------
BORDER_LONG = [b"abcd", b"abcde", b"aceghf", b"hgfedcb", b"gfedcbah", b"abcdefgh" * 2 + b"hgfedcb", b"abcdefgh" * 3, b"hgfe" * 7 + b"dc"]
BORDER_TERMS = [b"b", b"ab", b"cab", b"xab", b"de"] + BORDER_LONG       # lengths 1, 2, 3 | 4, 5, 6, 7, 8, 23, 24, 30
START_ENDS = [0, 1, 2, 3, 6, 7, 22, 23]
END_GAPS = [0, 1, 2, 3, 4]


@pytest.fixture(scope="module")
def border():
    plain = [po.lit(t) for t in BORDER_TERMS] + ['"cab" and not "abcd"', '"b" or "de"']
    h = Harness(BORDER_TERMS, plain, plain + ['inord("ab" and "b")'], once=True, slack=b"cdefghabcdexab")
    yield h
    h.close()


def _ending_at(end):
    """documents in which a term ENDS at offset `end`: every term that fits, behind filler and in front of a few bytes more"""
    out = []
    for t in BORDER_TERMS:
        if len(t) <= end + 1:
            out.append(po.fill(end + 1 - len(t)) + t + po.fill(9))
    return out


@pytest.mark.parametrize("mode", ["plain", "inord"])
def test_matches_that_end_in_the_first_bytes_of_the_blob(border, mode):
    """the blob's FIRST document: a match that ends at offset 0, 1, 2 (the short-term rule for p < 3), 3, 6, 7 (the window's
    8-byte load would start in front of the blob) and 22, 23 (the 16 bytes in front of the window would)"""
    assert [len(t) for t in BORDER_TERMS] == [1, 2, 3, 3, 2, 4, 5, 6, 7, 8, 23, 24, 30]
    seen = 0
    for end in START_ENDS:
        for first in _ending_at(end):
            blob, off = docs([first, b"", po.fill(30) + b"cab"])
            _, matches = border.process(mode, blob, off)
            seen += matches
            if mode == "inord":
                border.csr(blob, off)
    assert seen > 3 * len(START_ENDS)


@pytest.mark.parametrize("mode", ["plain", "inord"])
def test_matches_that_end_in_the_last_bytes_of_the_blob(border, mode):
    """the blob's LAST document: a keyword ends on the last byte and 1 to 4 bytes in front of it (the 4 bytes behind a window
    would reach past the blob: they read as zero, and the bytes behind the blob -- which spell terms here -- are never text)"""
    seen = 0
    for gap in END_GAPS:
        for t in BORDER_TERMS:
            for lead in (40, 0):
                last = po.fill(lead) + t + po.fill(gap)
                blob, off = docs([po.fill(50) + b"xab", b"", last])
                assert int(off[-1]) == blob.size
                _, matches = border.process(mode, blob, off)
                seen += matches
        if mode == "inord":
            border.csr(blob, off)
    assert seen > 3 * len(END_GAPS) * len(BORDER_TERMS)


# ---- empty inputs ---------------------------------------------------------------------------------------------------------
def test_zero_length_documents_between_others(border):
    """zero-length documents (each one an empty unit) first, last, in a row and between documents with matches"""
    full = po.fill(20) + b"abcde" + po.fill(3) + b"cab" + po.fill(70) + BORDER_LONG[-1]
    for texts in ([b"", full, b"", b"", full, b""], [b""], [b"", b""], [full, b"", b"b", b"", b"ab", b""]):
        blob, off = docs(texts)
        for step in ("plain", "inord", "plain"):
            border.process(step, blob, off)
        border.csr(blob, off)
