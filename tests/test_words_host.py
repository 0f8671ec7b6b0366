"""Whole-word matching on the host: gft_debug_word_rune against the alphabet of word_cases.py and against unicodedata, and
gft_debug_filter_word_matches -- the kernels' walk, entry tile by entry tile through the header the kernels compile -- against the
Python reference of word_cases.py on every neighbour kind, the document's and the walk's borders (from gft_debug_words_shape), both
length sources, positions of last bytes, the cap protocol, the refusals, which must leave every output byte as it was, and a seeded
random batch; tools/words_check.cpp built with the address and undefined-behaviour sanitizers and run.  All comparisons are exact;
no device needed."""
import ctypes as C
import os
import shutil
import subprocess
import unicodedata

import numpy as np
import pytest

import word_cases as W
from gofindthem_amd import _lib
from gofindthem_amd.engine import Engine, GftError, filter_word_matches_host, word_rune, words_shape

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gft_filter_word_matches_device", "gft_debug_filter_word_matches", "gft_debug_word_rune", "gft_debug_words_shape", "gft_scan_words_device",
         "gft_process_words_device", "gft_process_words", "gft_hit_spans_words_device", "gft_batch_term_stats_words_device",
         "gft_finder_set_whole_words", "gft_finder_whole_words")
SH = words_shape()
T = SH["tile_entries"]
NEIGHBOURS = W.neighbour_cases()
BORDERS = W.border_cases(T)
RANDOM = W.random_case()


def run(case, from_terms, **kw):
    """the host twin over a case: the lengths from the term table (from_terms) or from the entries"""
    return filter_word_matches_host(case.blob, case.doc_off, case.off, case.pos, None if from_terms else case.length, case.term,
                                    case.term_len if from_terms else None, case.pos_end, **kw)


def test_symbols_present():
    L = _lib.load()
    header = open(os.path.join(ROOT, "include", "gft.h")).read()
    for name in NAMES:
        assert hasattr(L, name) and name in _lib.SYMBOLS and name in header
    assert "GFT_WORDS_POS_END 1u" in header
    assert SH["table_rows"] == 126 and SH["table_bytes"] == 12736 and T % 64 == 0


def test_word_rune_ascii_and_alphabet():
    for cp in range(128):
        assert word_rune(cp) == (chr(cp).isalnum() or chr(cp) == "_"), cp
    for cp, want in W.CLASS.items():
        assert word_rune(cp) == want, hex(cp)
    for cp in (0xD800, 0xDBFF, 0xDC00, 0xDFFF, 0xFFFD, 0x110000, 0x110001, 0x7FFFFFFF, 0xFFFFFFFF):
        assert not word_rune(cp), hex(cp)


def test_word_rune_every_code_point():
    inc = open(os.path.join(ROOT, "gofindthem_amd", "csrc", "unicode_word.inc")).readline()
    assert "unicodedata" in inc
    version = inc.split("unicodedata")[1].split()[0]
    if version != unicodedata.unidata_version:
        pytest.skip("the table was generated from Unicode %s, this interpreter has %s" % (version, unicodedata.unidata_version))
    L = _lib.load()
    for cp in range(0x110000):
        cat = unicodedata.category(chr(cp))
        assert bool(L.gft_debug_word_rune(cp)) == (cat[0] in "LMN" or cat == "Pc"), hex(cp)


@pytest.mark.parametrize("case", NEIGHBOURS + BORDERS, ids=[c.name for c in NEIGHBOURS + BORDERS])
@pytest.mark.parametrize("from_terms", [True, False], ids=["term_len", "entry_len"])
def test_cases(case, from_terms):
    W.check_outputs(case, *run(case, from_terms, guard=3), guard=3)


def test_sentence_table():
    case = BORDERS[0]
    total, out_off, pos, length, term = run(case, True)
    got = {}
    for p, t in zip(pos[:total], term[:total]):
        got.setdefault(case.terms[t], []).append(int(p))
    assert got == W.SENTENCE_KEPT


def test_random_batch():
    kept = sum(RANDOM.keep)
    print("random batch: %d occurrences, %d kept, %d dropped" % (RANDOM.n, kept, RANDOM.n - kept))
    assert kept > 500 and RANDOM.n - kept > 500                    # both outcomes are exercised
    for from_terms in (True, False):
        W.check_outputs(RANDOM, *run(RANDOM, from_terms, guard=2), guard=2)


@pytest.mark.parametrize("name", ["sentence", "tile_%d" % (T + 1), "pos_end"])
def test_cap_protocol(name):
    case = next(c for c in BORDERS if c.name == name)
    total = sum(case.keep)
    for cap in (0, 1, total - 1, total, total + 5):
        W.check_outputs(case, *run(case, True, cap=cap, guard=4), cap=cap, guard=4)
    # count only: every output NULL
    n = C.c_uint64(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)                      # noqa: E731
    rc = _lib.load().gft_debug_filter_word_matches(p(case.blob), p(case.doc_off), case.n_docs, p(case.off), p(case.pos), None, p(case.term),
                                                   p(case.term_len), len(case.terms), 1 if case.pos_end else 0, None, None, None, None, 0, C.byref(n))
    assert rc == 0 and n.value == total
    # each of len and term dropped on its own
    for wl, wt in ((False, True), (True, False), (False, False)):
        W.check_outputs(case, *run(case, True, with_len=wl, with_term=wt, guard=1), guard=1)


def refusal_inputs():
    """(name, case, from_terms, the arrays to break as a function of copies): what the check pass must find"""
    base = next(c for c in BORDERS if c.name == "straddle")

    def descending(c):
        c.off[2] = c.off[1] - 1

    def bad_term(c):
        c.term[c.n - 1] = len(c.terms)

    def past_doc(c):
        c.pos[T - 4] = len(c.docs[0]) - 1                           # the last entry of document 0 now ends one byte behind it

    def before_doc(c):
        c.pos_end, c.pos[0] = True, 0                               # an entry of two bytes whose last byte is the document's first

    def flags(c):
        c.flags = 6

    return [("descending_offset", base, True, descending), ("term_out_of_range", base, True, bad_term), ("entry_past_document", base, True, past_doc),
            ("entry_past_document_entry_len", base, False, past_doc), ("entry_before_document", base, True, before_doc), ("unknown_flags", base, True, flags)]


REFUSALS = refusal_inputs()


@pytest.mark.parametrize("r", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(r):
    import copy
    name, case, from_terms, breaker = r
    c = copy.deepcopy(case)
    c.flags = None
    breaker(c)
    L = _lib.load()
    p = lambda a: a.ctypes.data_as(C.c_void_p)                      # noqa: E731
    outs = [np.full(c.n_docs + 1, 0x5A5A5A5A5A5A5A5A, np.uint64)] + [np.full(c.n, 0x5A5A5A5A, np.uint32) for _ in range(3)]
    n = C.c_uint64(77)
    fl = c.flags if c.flags is not None else (1 if c.pos_end else 0)
    rc = L.gft_debug_filter_word_matches(p(c.blob), p(c.doc_off), c.n_docs, p(c.off), p(c.pos), None if from_terms else p(c.length), p(c.term),
                                         p(c.term_len) if from_terms else None, len(c.terms) if from_terms else 0, fl, *(p(o) for o in outs),
                                         c.n, C.byref(n))
    assert rc == W.E_INVALID and n.value == 0
    assert (outs[0] == 0x5A5A5A5A5A5A5A5A).all() and all((o == 0x5A5A5A5A).all() for o in outs[1:])


def test_overlaps():
    """an output that overlaps an input or another output: refused, nothing written"""
    L = _lib.load()
    case = next(c for c in BORDERS if c.name == "tile_%d" % T)
    p = lambda a: a.ctypes.data_as(C.c_void_p)                      # noqa: E731
    pool = np.full(4 * case.n + 64, 0x77777777, np.uint32)
    pos, term = case.pos.copy(), case.term.copy()
    views = {"pos_over_pos": (None, pos, None, None), "len_over_term": (None, pool[:case.n], term, None),
             "pos_and_len": (None, pool[:case.n], pool[case.n - 1:2 * case.n - 1], None),
             "off_over_pos": (pos[:2 * (case.n_docs + 1)].view(np.uint64), pool[:case.n], None, None),
             "pos_over_text": (None, case.blob[:(case.blob.size // 4) * 4].view(np.uint32), None, None)}
    for name, (oo, a, b, c) in views.items():
        keep = (pool.copy(), pos.copy(), term.copy(), case.blob.copy())
        cap = min(case.n, a.size)
        rc = L.gft_debug_filter_word_matches(p(case.blob), p(case.doc_off), case.n_docs, p(case.off), p(pos), None, p(term), p(case.term_len),
                                             len(case.terms), 0, p(oo) if oo is not None else None, p(a), p(b) if b is not None else None,
                                             p(c) if c is not None else None, cap, None)
        assert rc == W.E_INVALID, name
        assert (pool == keep[0]).all() and (pos == keep[1]).all() and (term == keep[2]).all() and (case.blob == keep[3]).all(), name


def test_engine_wrapper():
    case = BORDERS[0]
    out_off, pos, length, term = Engine.filter_word_matches_host(case.blob, case.doc_off, case.off, case.pos, None, case.term, case.term_len)
    w_off, w_pos, w_len, w_term = case.reference()
    assert (out_off == w_off).all() and (pos == w_pos).all() and (length == w_len).all() and (term == w_term).all()
    assert Engine.words_shape() == SH
    with pytest.raises(GftError):
        filter_word_matches_host(case.blob, case.doc_off, case.off, case.pos, None, case.term, case.term_len, flags=2)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_words_check_under_sanitizers(tmp_path):
    exe = str(tmp_path / "words_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", ROOT,
           os.path.join(ROOT, "tools", "words_check.cpp"), os.path.join(ROOT, "gofindthem_amd", "csrc", "words_host.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, cwd=ROOT)
    r = subprocess.run([exe, "60"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
