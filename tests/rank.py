"""Shared by test_rank_host.py and test_gpu_rank.py: the cases of the score, top and gather calls, references in plain numpy written
from the contract alone (prefix sums of the weights, unique over (document, term) pairs for the distinct mode, lexsort for the order --
no code of the piece header), and the checks themselves, which take a runner: a callable with the C call's arguments over numpy
arrays that fills the outputs in place and returns (status, the call's host result).  The host file runs them through
gft_debug_score_docs / gft_debug_top_docs / gft_debug_gather_docs, the GPU file through the device calls.  The borders come from
gft_debug_rank_shape and gft_debug_select_shape."""
import numpy as np

from term_stats import Case, small, zipf_docs

MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
DISTINCT = 1
E_INVALID = -1
PATTERN = np.uint64(0x5A5A5A5A5A5A5A5A)
BASE = (1 << 40) + 5                  # a doc_base above 2^40


# ---- scores -------------------------------------------------------------------------------------------------------------------

def score_reference(off, term, n_docs, n_terms, weights=None, distinct=False):
    score = np.zeros(n_docs, np.uint64)
    if not n_docs:
        return score
    o = np.asarray(off[:n_docs + 1], dtype=np.int64)
    t = np.asarray(term[o[0]:o[-1]], dtype=np.int64)
    if not t.size:
        return score
    w = np.ones(n_terms, np.uint64) if weights is None else np.asarray(weights, dtype=np.uint64)
    if distinct:
        doc = np.repeat(np.arange(n_docs, dtype=np.int64), np.diff(o))
        pairs = np.unique(np.stack([doc, t], axis=1), axis=0)
        np.add.at(score, pairs[:, 0], w[pairs[:, 1]])
        return score
    c = np.concatenate([np.zeros(1, np.uint64), np.cumsum(w[t], dtype=np.uint64)])
    return c[o[1:] - o[0]] - c[o[:-1] - o[0]]


def score_cases(sh):
    """Case objects with .weights (None or uint32 [n_terms]) and .modes (the flags to run)"""
    S, B, SD, SS, LT, WL, RW = (sh[k] for k in ("step_entries", "large_entries", "step_docs", "set_slots", "bitset_lds_terms", "weight_lds_terms",
                                               "range_weight"))
    rng = np.random.default_rng(20261021)
    two = lambda n: np.arange(n) % 2 * 3 + 1                        # noqa: E731  (terms 1 and 4, alternating)
    cs = []

    def add(name, docs, n_terms, weights="random", modes=(0, DISTINCT), lead=0, tail=0):
        c = Case(name, docs, n_terms, lead=lead, tail=tail)
        c.weights = rng.integers(0, 1000, n_terms).astype(np.uint32) if isinstance(weights, str) else weights
        c.modes = modes
        cs.append(c)
    for n in (S - 1, S, S + 1):
        add("one_doc_%d" % n, [np.arange(n) % 7], 11)
    for n in (S - 1, S, S + 1):
        k, rem = divmod(n, 5)
        add("step_sum_%d" % n, small(rng, [5] * k + ([rem] if rem else []) + [5] * 40, 23), 23)
    for n in (B - 1, B, B + 1):
        add("large_%d" % n, [two(n)], 6)
    add("large_between_small", small(rng, [3, 0, 7, 2], 9) + [two(B + 17)] + small(rng, [4, 4, 0, 1], 9), 9)
    add("two_large", [two(B + 3), two(2 * S + 5) + 1], 9)
    add("large_then_step", [two(3 * S)] + small(rng, [2] * 30, 9), 9)
    add("empty_runs", [[]] * 5 + small(rng, [2], 9) + [[]] * (SD + 3) + small(rng, [3], 9) + [[]] * 2, 9)
    add("empty_batch_long", [[]] * (2 * SD + 1), 9)
    add("no_docs", [], 9)
    add("no_terms", [[], []], 0)
    add("off0", small(rng, [4, 0, 9, 3], 9), 9, lead=13, tail=5)
    add("cut_middle", small(rng, [6] * 300, 31), 31, lead=777, tail=99)
    add("step_docs", small(rng, [1] * (SD + 1), 5) + small(rng, [0, 1] * SD, 5), 5)
    k = (RW - 20) // 8
    add("ranges", small(rng, [7] * k, 29) + [two(B + 5)] + small(rng, [7] * (4 * k), 29), 29)
    add("ranges_lines", small(rng, rng.integers(0, 4, 6 * RW // 2), 301), 301)
    add("weights_zero", small(rng, [5] * 50, 9) + [two(B + 1)], 9, weights=np.zeros(9, np.uint32))
    add("weights_one_muted", small(rng, [5] * 50, 4) + [np.arange(B + 9) % 4], 4, weights=np.array([3, 0, 0xFFFFFFFF, 1], np.uint32))
    # weights of 2^32 - 1 on a large document: the sum passes 2^32 -- the carry is the point
    add("carry_large", small(rng, [3, 3], 6) + [two(B + 40)], 6, weights=np.full(6, 0xFFFFFFFF, np.uint32))
    add("carry_step", small(rng, [9] * 100, 6), 6, weights=np.full(6, 0xFFFFFFFF, np.uint32))
    same = small(rng, [5] * 300, 40) + [two(B + 3)]
    add("weights_null", same, 40, weights=None)
    add("weights_ones", same, 40, weights=np.ones(40, np.uint32))
    add("set_collide", [[5, 5 + SS, 5 + 2 * SS, 5, 5 + SS]] * 150 + [[5 + SS, 5]] * 150, 3 * SS)
    for nt in (LT - 1, LT, LT + 1):
        d = two(B + 9).copy()
        d[5::7] = nt - 1                                            # the highest term id, again and again
        add("bitset_%d" % nt, small(rng, [3, 3], nt) + [d] + [[nt - 1, 0, nt - 1]], nt)
    for nt in (WL - 1, WL, WL + 1):
        d = (np.arange(B + 30) * 37) % nt
        d[3::11] = nt - 1
        add("weights_lds_%d" % nt, small(rng, [4] * 60, nt) + [d] + [[nt - 1, 0, nt - 1, nt - 1]], nt)
    for i in range(6):
        r = np.random.default_rng(4200 + i)
        n_terms = int(r.choice([3, 50, 1000, 5000, WL + 3]))
        docs = (zipf_docs(r, int(r.integers(1, 900)), n_terms, 4.0), zipf_docs(r, int(r.integers(1, 12)), n_terms, S * 0.6),
                zipf_docs(r, 200, n_terms, 2.0) + zipf_docs(r, 2, n_terms, 1.5 * S) + zipf_docs(r, 300, n_terms, 6.0))[i % 3]
        add("zipf_%d" % i, docs, n_terms, lead=int(r.integers(0, 50)), tail=int(r.integers(0, 50)))
    return cs


def check_score(run, case):
    """run(off, term, n_docs, n_terms, weights, flags, score) -> (status, max_score); every score is written"""
    for flags in case.modes:
        score = np.full(case.n_docs, PATTERN, np.uint64)
        rc, mx = run(case.off, case.term, case.n_docs, case.n_terms, case.weights, flags, score)
        assert rc == 0, case.name
        want = score_reference(case.off, case.term, case.n_docs, case.n_terms, case.weights, bool(flags & DISTINCT))
        bad = np.nonzero(score != want)[0]
        assert not bad.size, "%s flags %d: score[%d] = %d, expected %d (%d differ)" % (case.name, flags, bad[0], score[bad[0]], want[bad[0]], bad.size)
        assert mx == (int(want.max()) if want.size else 0), (case.name, flags)


def check_null_weights_are_ones(run, cases):
    """weights == NULL against explicit ones, on the same list"""
    a, b = (next(c for c in cases if c.name == n) for n in ("weights_null", "weights_ones"))
    for flags in (0, DISTINCT):
        sa, sb = np.zeros(a.n_docs, np.uint64), np.zeros(b.n_docs, np.uint64)
        assert run(a.off, a.term, a.n_docs, a.n_terms, a.weights, flags, sa)[0] == 0 and a.weights is None
        assert run(b.off, b.term, b.n_docs, b.n_terms, b.weights, flags, sb)[0] == 0
        assert (sa == sb).all() and sa.any()


def score_refusals(sh):
    """(name, off, term, n_docs, n_terms, flags): every one is GFT_E_INVALID"""
    S = sh["step_entries"]
    rng = np.random.default_rng(3)
    base = Case("base", small(rng, [5] * (S // 2), 40), 40)
    out = []
    t = base.term.copy(); t[len(t) // 2] = 40
    out.append(("term_eq_n_terms", base.off, t, base.n_docs, 40, 0))
    t = base.term.copy(); t[-1] = 0xFFFFFFFF
    out.append(("term_max_last", base.off, t, base.n_docs, 40, DISTINCT))
    o = base.off.copy(); o[base.n_docs // 2] -= np.uint64(7)
    out.append(("offset_descends", o, base.term, base.n_docs, 40, 0))
    o = base.off.copy(); o[-1] = 0; o[0] = 5
    out.append(("ends_descend", o, base.term, base.n_docs, 40, 0))
    out.append(("unknown_flags", base.off, base.term, base.n_docs, 40, 2))
    out.append(("unknown_flags_high", base.off, base.term, base.n_docs, 40, DISTINCT | 0x80000000))
    out.append(("entries_no_terms", base.off, base.term, base.n_docs, 0, 0))
    return out


def check_score_refusal(run, off, term, n_docs, n_terms, flags):
    score = np.full(n_docs, PATTERN, np.uint64)
    assert run(off, term, n_docs, n_terms, np.ones(max(n_terms, 1), np.uint32), flags, score)[0] == E_INVALID
    assert (score == PATTERN).all(), "a refused call wrote"


# ---- the top list -------------------------------------------------------------------------------------------------------------

def top_reference(score, k, doc_base=0):
    s = np.asarray(score, dtype=np.uint64)
    nz = np.nonzero(s)[0]
    order = nz[np.lexsort((nz, MAX - s[nz]))][:k]
    return order.astype(np.uint64) + np.uint64(doc_base), s[order]


def top_cases(sh):
    """(name, scores uint64, the ks to ask for)"""
    PT, K = sh["place_tile"], sh["max_k"]
    rng = np.random.default_rng(77)
    u64 = lambda a: np.asarray(a, dtype=np.uint64)                  # noqa: E731
    cs = []
    for k in (1, 63, 64, 65, K):
        for n in sorted({max(k - 1, 1), k, k + 1, 3 * k + 7}):
            s = rng.integers(0, 40, n).astype(np.uint64)            # many ties, some zeros
            cs.append(("k%d_n%d" % (k, n), s, (k,)))
    cs.append(("all_equal", np.full(3 * PT + 5, 9, np.uint64), (1, 65, PT + 1, K)))
    cs.append(("all_zero", np.zeros(2 * PT + 1, np.uint64), (1, 64, K)))
    s = np.zeros(3 * PT, np.uint64); s[rng.choice(3 * PT, 63, replace=False)] = rng.integers(1, 5, 63).astype(np.uint64)
    cs.append(("k_minus_1_nonzero", s, (64,)))
    # a threshold value shared by many more documents than r: the equals in every tile, across the tiles' and the workgroups' borders
    s = np.full(5 * PT + 77, 3, np.uint64); s[::50] = 7; s[[5, PT - 1, PT, 2 * PT + 1, 4 * PT, 5 * PT + 76, 17, 3 * PT - 1, 900, 2]] = u64(range(100, 110))
    cs.append(("shared_threshold", s, (64, 11, 10, 12)))
    s = rng.integers(1, 3, 10 * PT + 3).astype(np.uint64); s[::2] = 5; s[rng.choice(s.size, 100, replace=False)] = 1000
    cs.append(("shared_threshold_wide", s, (K, 101, 100)))
    s = np.uint64(0x0123456789ABCD00) + u64(rng.integers(0, 256, 2 * PT + 9))
    cs.append(("lowest_digit", s, (1, 64, 700)))
    s = u64(rng.integers(1, 201, 2 * PT + 9)) << np.uint64(56)
    cs.append(("highest_digit", s, (1, 64, 700)))
    s = u64([int(MAX), 1 << 32, (1 << 32) - 1, (1 << 32) + 1, 0, int(MAX), 1, int(MAX) - 1, 1 << 63, (1 << 63) - 1] * 30)
    cs.append(("extremes", s, (1, 3, 64, 65, 299)))
    s = rng.integers(0, 1 << 63, 4 * PT + 11, dtype=np.int64).astype(np.uint64) * np.uint64(2) + u64(rng.integers(0, 2, 4 * PT + 11))
    cs.append(("random_words", s, (1, 10, 65, K)))
    s = rng.integers(0, 1 << 20, 150000).astype(np.uint64)          # several histogram workgroups, ties at the threshold
    cs.append(("many_docs", s, (10, K)))
    cs.append(("no_docs", np.zeros(0, np.uint64), (0, 5)))
    cs.append(("k_zero", u64([4, 5, 6]), (0,)))
    return cs


def check_top(run, name, score, k, doc_base=BASE):
    """run(score, n_docs, k, doc_base, top_idx, top_score) -> (status, n_top); the entries at and past n_top keep the pattern"""
    ti, ts = np.full(k + 3, PATTERN, np.uint64), np.full(k + 3, PATTERN + np.uint64(1), np.uint64)
    rc, n = run(score, score.size, k, doc_base, ti, ts)
    assert rc == 0, name
    wi, wv = top_reference(score, k, doc_base)
    assert n == wi.size == min(k, int(np.count_nonzero(score))), (name, k, n)
    assert (ti[:n] == wi).all() and (ts[:n] == wv).all(), (name, k)
    assert (ti[n:] == PATTERN).all() and (ts[n:] == PATTERN + np.uint64(1)).all(), (name, k, "written past n_top")


# ---- the gather ---------------------------------------------------------------------------------------------------------------

def gather_batch(select_shape):
    """(blob uint8 with 64 bytes of slack, doc_off): documents whose lengths stand at the copy kernel's chunk, trip and tile borders,
    documents of 0 bytes among them, in front of a text that does not begin at 0"""
    chunk, trip, tile = select_shape
    rng = np.random.default_rng(5)
    lens = [0, 1, chunk - 1, chunk, chunk + 1, 0, 0, trip - 1, trip, trip + 1, 3, tile - 1, tile, tile + 1, 0, 2 * tile + 5, 7, 0]
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    off += np.uint64(9)                                             # (doc_off[0] != 0)
    blob = rng.integers(1, 255, int(off[-1]) + 64).astype(np.uint8)
    return blob, off


def gather_lists(n_docs):
    rng = np.random.default_rng(6)
    ident = np.arange(n_docs, dtype=np.uint64)
    empties = np.array([0, 5, 6, 14, 17], dtype=np.uint64)
    return [("identity", ident), ("reversed", ident[::-1].copy()), ("repeats", np.array([3, 3, 3, 15, 0, 15, 3, 8, 8], np.uint64)),
            ("empty", np.zeros(0, np.uint64)), ("zero_byte_docs", empties), ("one", np.array([12], np.uint64)),
            ("random", rng.integers(0, n_docs, 70).astype(np.uint64))]


def gather_reference(blob, off, idx, idx_base=0):
    d = (np.asarray(idx, dtype=np.uint64) - np.uint64(idx_base)).astype(np.int64)
    parts = [blob[int(off[i]):int(off[i + 1])] for i in d]
    lens = np.array([p.size for p in parts], dtype=np.uint64)
    out_off = np.zeros(len(parts) + 1, np.uint64)
    out_off[1:] = np.cumsum(lens)
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)), out_off


def check_gather(run, blob, off, name, idx, idx_base=0):
    """run(blob, doc_off, n_docs, idx, idx_base, out or None, cap_bytes, out_off) -> (status, total); out has guard bytes behind
    cap_bytes, out_off guard entries behind m + 1: every cap cut is byte-exact"""
    n_docs, m = off.size - 1, idx.size
    want, want_off = gather_reference(blob, off, idx)
    shifted = idx + np.uint64(idx_base)
    total = want.size
    for cap in sorted({total, max(total - 1, 0), total // 2, 1 if total else 0, 0, total + 9}):
        out = np.full(cap + 32, 0xA5, np.uint8)
        out_off = np.full(m + 1 + 4, PATTERN, np.uint64)
        rc, tot = run(blob, off, n_docs, shifted, idx_base, out if cap else None, cap, out_off)
        assert rc == 0 and tot == total, (name, cap)
        assert (out_off[:m + 1] == want_off).all() and (out_off[m + 1:] == PATTERN).all(), (name, cap)
        w = min(cap, total)
        assert (out[:w] == want[:w]).all(), (name, cap)
        assert (out[w:] == 0xA5).all(), (name, cap, "stored at or past min(total, cap_bytes)")


def check_gather_refusals(run, blob, off):
    n_docs = off.size - 1
    for name, bad in (("n_docs", n_docs + 7), ("max", int(MAX)), ("below_base", 6)):
        idx = np.array([8, 9, bad, 10], np.uint64)
        out, out_off = np.full(64, 0xA5, np.uint8), np.full(5, PATTERN, np.uint64)
        rc, _ = run(blob, off, n_docs, idx, 7, out, 64, out_off)
        assert rc == E_INVALID, name
        assert (out == 0xA5).all() and (out_off == PATTERN).all(), name
