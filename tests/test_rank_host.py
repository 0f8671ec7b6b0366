"""The ranking calls on the host: gft_debug_score_docs, gft_debug_top_docs and gft_debug_gather_docs -- the kernels' walks step by step
and lane by lane through the header the kernels compile -- against the numpy references of rank.py on the cases at the walks'
borders (from gft_debug_rank_shape and gft_debug_select_shape): every path of the score walk in both modes, the 64-bit carry, NULL
weights, the select at every k that matters with ties at the threshold across tiles, the gather at every cap cut, the refusals,
which must leave every output byte for byte, and the overlaps; tools/rank_check.cpp built with the address and undefined-behaviour
sanitizers and run as a program of its own.  All comparisons are exact; no device needed."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import rank as RK
from gofindthem_amd import _lib
from gofindthem_amd.engine import Engine, GftError, gather_docs_host, rank_shape, score_docs_host, select_shape, top_docs_host

NAMES = ("gft_score_docs_device", "gft_top_docs_device", "gft_gather_docs_device", "gft_batch_top_docs_device", "gft_batch_top_docs_words_device",
         "gft_debug_score_docs", "gft_debug_top_docs", "gft_debug_gather_docs", "gft_debug_rank_shape", "gft_finder_top_docs_device")
SH = rank_shape()
SCORE = RK.score_cases(SH)
TOP = RK.top_cases(SH)
BLOB, OFF = RK.gather_batch(select_shape())
LISTS = RK.gather_lists(OFF.size - 1)
REFUSALS = RK.score_refusals(SH)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None      # noqa: E731


def run_score(off, term, n_docs, n_terms, weights, flags, score):
    try:
        return 0, score_docs_host(off, term, n_terms, weights, score=score, flags=flags, n_docs=n_docs)[1]
    except GftError as e:
        return e.code, 0


def run_top(score, n_docs, k, doc_base, top_idx, top_score):
    try:
        return 0, top_docs_host(score, k, doc_base, top_idx, top_score, n_docs=n_docs)
    except GftError as e:
        return e.code, 0


def run_gather(blob, off, n_docs, idx, idx_base, out, cap, out_off):
    total = C.c_uint64(0)
    rc = _lib.load().gft_debug_gather_docs(p(blob), p(off), n_docs, p(idx), idx.size, idx_base, out.ctypes.data if out is not None else None, cap,
                                           out_off.ctypes.data, C.byref(total))
    return rc, int(total.value)


def test_symbols_present():
    L = _lib.load()
    header = open(_lib.__file__.replace("gofindthem_amd/_lib.py", "include/gft.h")).read()
    for name in NAMES:
        assert hasattr(L, name) and name in _lib.SYMBOLS and name in header
    assert "GFT_SCORE_DISTINCT 1u" in header and _lib.GFT_SCORE_DISTINCT == RK.DISTINCT
    assert SH["large_entries"] == SH["step_entries"] + 1 and SH["max_k"] == 4096 and 64 % SH["digit_bits"] == 0
    assert SH["place_tile"] % 64 == 0 and SH["weight_lds_terms"] >= 1024


@pytest.mark.parametrize("case", SCORE, ids=[c.name for c in SCORE])
def test_score(case):
    RK.check_score(run_score, case)


def test_null_weights_are_ones():
    RK.check_null_weights_are_ones(run_score, SCORE)


@pytest.mark.parametrize("r", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_score_refusals(r):
    RK.check_score_refusal(run_score, *r[1:])


@pytest.mark.parametrize("c", TOP, ids=[c[0] for c in TOP])
def test_top(c):
    name, score, ks = c
    for k in ks:
        RK.check_top(run_top, name, score, k)
    RK.check_top(run_top, name, score, ks[0], doc_base=0)


def test_top_refusals():
    score = np.arange(1, 9000, dtype=np.uint64)
    ti, ts = np.full(5000, RK.PATTERN, np.uint64), np.full(5000, RK.PATTERN, np.uint64)
    assert run_top(score, score.size, SH["max_k"] + 1, 0, ti, ts)[0] == RK.E_INVALID
    assert (ti == RK.PATTERN).all() and (ts == RK.PATTERN).all()
    RK.check_top(run_top, "after", score, SH["max_k"])


@pytest.mark.parametrize("lst", LISTS, ids=[n for n, _ in LISTS])
def test_gather(lst):
    RK.check_gather(run_gather, BLOB, OFF, *lst)
    RK.check_gather(run_gather, BLOB, OFF, lst[0], lst[1], idx_base=(1 << 40) + 1)


def test_gather_unaligned_outputs():
    """the copy's chunks follow the output's address: every offset into the 16-byte grid"""
    want, want_off = RK.gather_reference(BLOB, OFF, LISTS[0][1])
    for shift in range(16):
        total, out, out_off = gather_docs_host(BLOB, OFF, LISTS[0][1], guard=8, out_shift=shift)
        assert total == want.size and (out[:total] == want).all() and (out[total:] == 0xA5).all() and (out_off[:want_off.size] == want_off).all()


def test_gather_refusals():
    RK.check_gather_refusals(run_gather, BLOB, OFF)
    RK.check_gather(run_gather, BLOB, OFF, *LISTS[2])


def test_overlaps():
    """an output that overlaps an input or the other output: refused, nothing written"""
    L = _lib.load()
    case = next(c for c in SCORE if c.name == "cut_middle")
    off, term = case.off.copy(), case.term.copy()
    keep_o, keep_t = off.copy(), term.copy()
    n = case.n_docs
    # (off[n:] is one word: the scores' first word on the offsets' last)
    for name, out in (("offsets", off[1:1 + n]), ("offsets_last_word", off[n:]), ("entries", term[778:778 + 2 * n].view(np.uint64))):
        assert L.gft_debug_score_docs(p(off), p(term), n, case.n_terms, None, 0, p(out), None) == RK.E_INVALID, name
        assert (off == keep_o).all() and (term == keep_t).all()
    # (the garbage in front of off[0] is no input: the scores may lie there)
    front = term[:2 * n].view(np.uint64)
    assert 2 * n <= 777 and L.gft_debug_score_docs(p(off), p(term), n, case.n_terms, None, 0, p(front), None) == 0
    # the top arrays over the scores and over each other
    pool = np.arange(1, 301, dtype=np.uint64)
    keep = pool.copy()
    nt = C.c_uint64(0)
    for name, (ti, ts) in {"idx_scores": (pool[90:], pool[200:]), "score_scores": (pool[200:], pool[95:]), "idx_score": (pool[100:], pool[105:])}.items():
        assert L.gft_debug_top_docs(p(pool), 100, 10, 0, p(ti), p(ts), C.byref(nt)) == RK.E_INVALID, name
        assert (pool == keep).all()
    assert L.gft_debug_top_docs(p(pool), 100, 10, 0, p(pool[100:]), p(pool[110:]), C.byref(nt)) == 0 and nt.value == 10
    # the gather's outputs over the text, the offsets, the list and each other
    blob, doff = BLOB.copy(), OFF.copy()
    idx = np.arange(4, dtype=np.uint64)
    spare, spare_off = np.zeros(64, np.uint8), np.zeros(8, np.uint64)
    tot = C.c_uint64(0)
    lo = int(doff[0])
    start = (-(blob.ctypes.data + lo)) % 8 + lo                     # (an aligned uint64 view inside the text)
    sets = {"out_text": (blob[lo + 8:], spare_off), "out_offsets": (doff.view(np.uint8)[8:], spare_off), "out_list": (idx.view(np.uint8), spare_off),
            "off_text": (spare, blob[start:start + 64].view(np.uint64)), "off_offsets": (spare, doff[2:]), "off_list": (spare, idx),
            "out_off": (spare_off.view(np.uint8), spare_off)}
    kb, ko, ki = blob.copy(), doff.copy(), idx.copy()
    for name, (out, oo) in sets.items():
        rc = L.gft_debug_gather_docs(p(blob), p(doff), doff.size - 1, p(idx), 4, 0, out.ctypes.data_as(C.c_void_p), 16, oo.ctypes.data_as(C.c_void_p),
                                     C.byref(tot))
        assert rc == RK.E_INVALID, name
        assert (blob == kb).all() and (doff == ko).all() and (idx == ki).all(), name
    # (the bytes in front of doc_off[0] are no input)
    assert L.gft_debug_gather_docs(p(blob), p(doff), doff.size - 1, p(idx), 4, 0, p(blob[:lo]), lo, p(spare_off), C.byref(tot)) == 0


def test_engine_wrappers():
    case = SCORE[0]
    score, mx = Engine.score_docs_host(case.off, case.term, case.n_terms, case.weights, distinct=True)
    want = RK.score_reference(case.off, case.term, case.n_docs, case.n_terms, case.weights, True)
    assert (score == want).all() and mx == int(want.max())
    name, s, ks = next(c for c in TOP if c[0] == "shared_threshold")
    ti, ts = Engine.top_docs_host(s, ks[0], 7)
    wi, wv = RK.top_reference(s, ks[0], 7)
    assert (ti == wi).all() and (ts == wv).all()
    out, out_off = Engine.gather_docs_host(BLOB, OFF, LISTS[1][1])
    want, want_off = RK.gather_reference(BLOB, OFF, LISTS[1][1])
    assert (out == want).all() and (out_off[:want_off.size] == want_off).all()
    assert Engine.rank_shape() == SH


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_rank_check_under_sanitizers(tmp_path):
    exe = str(tmp_path / "rank_check")
    csrc = os.path.join(ROOT, "gofindthem_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", ROOT,
           os.path.join(ROOT, "tools", "rank_check.cpp"), os.path.join(csrc, "rank_host.cpp"), os.path.join(csrc, "select_host.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, cwd=ROOT)
    r = subprocess.run([exe, "40"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
