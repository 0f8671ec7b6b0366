"""Shared by test_term_stats_host.py and test_gpu_term_stats.py: the cases of the term statistics and the column counts, a reference
in plain numpy written from the contract alone (bincount, and unique over (document, term) pairs -- no code of the piece header),
and the checks themselves, which take a runner: a callable with the C call's arguments over numpy arrays that fills the outputs in
place and returns the status.  The host file runs them through gft_debug_term_stats / gft_debug_count_columns, the GPU file through
the device calls.  The borders come from gft_debug_stats_shape."""
import numpy as np

MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
ACC = 1
E_INVALID = -1
GARBAGE = 0xFFFFFFFF          # what lies in front of off[0] and behind off[n]: never read, never checked


class Case:
    def __init__(self, name, docs, n_terms, lead=0, tail=0):
        """docs: a list of sequences of term ids; lead / tail: entries of garbage in front of and behind the list"""
        self.name, self.n_terms, self.n_docs = name, int(n_terms), len(docs)
        sizes = np.array([len(d) for d in docs], dtype=np.uint64)
        self.off = np.zeros(len(docs) + 1, dtype=np.uint64)
        self.off[1:] = np.cumsum(sizes)
        self.off += np.uint64(lead)
        body = np.concatenate([np.asarray(d, dtype=np.uint32) for d in docs]) if docs and sizes.sum() else np.zeros(0, np.uint32)
        self.term = np.concatenate([np.full(lead, GARBAGE, np.uint32), body, np.full(tail, GARBAGE, np.uint32)])


def reference(off, term, n_docs, n_terms, doc_base=0):
    """(occ, docs, first) of the contract"""
    occ, docs = np.zeros(n_terms, np.uint64), np.zeros(n_terms, np.uint64)
    first = np.full(n_terms, MAX, np.uint64)
    if not n_docs:
        return occ, docs, first
    o = np.asarray(off[:n_docs + 1], dtype=np.int64)
    t = np.asarray(term[o[0]:o[-1]], dtype=np.int64)
    if not t.size:
        return occ, docs, first
    occ = np.bincount(t, minlength=n_terms).astype(np.uint64)
    doc = np.repeat(np.arange(n_docs, dtype=np.int64), np.diff(o))
    pairs = np.unique(np.stack([doc, t], axis=1), axis=0)
    docs = np.bincount(pairs[:, 1], minlength=n_terms).astype(np.uint64)
    np.minimum.at(first, pairs[:, 1], (pairs[:, 0] + doc_base).astype(np.uint64))
    return occ, docs, first


def zipf_docs(rng, n_docs, n_terms, mean, a=1.3, max_len=None):
    docs = []
    for _ in range(n_docs):
        k = int(rng.poisson(mean)) if max_len is None else min(int(rng.poisson(mean)), max_len)
        docs.append((rng.zipf(a, k) - 1) % n_terms)
    return docs


def small(rng, sizes, n_terms):
    return [rng.integers(0, n_terms, int(k)) for k in sizes]


def fixed_cases(sh):
    S, B, SD, CS, SS, LT, RW = (sh[k] for k in ("step_entries", "large_entries", "step_docs", "cache_slots", "set_slots", "bitset_lds_terms",
                                                "range_weight"))
    rng = np.random.default_rng(20261020)
    two = lambda n: np.arange(n) % 2 * 3 + 1                        # noqa: E731  (terms 1 and 4, alternating)
    cs = []
    for n in (S - 1, S, S + 1):
        cs.append(Case("one_doc_%d" % n, [np.arange(n) % 7], 11))
    for n in (S - 1, S, S + 1):
        # documents of 5 entries (and one remainder) that end a step at exactly n entries, then more of them
        k, rem = divmod(n, 5)
        cs.append(Case("step_sum_%d" % n, small(rng, [5] * k + ([rem] if rem else []) + [5] * 40, 23), 23))
    for n in (B - 1, B, B + 1):
        cs.append(Case("two_terms_%d" % n, [two(n)], 6))
    cs.append(Case("large_between_small", small(rng, [3, 0, 7, 2], 9) + [two(B + 17)] + small(rng, [4, 4, 0, 1], 9), 9))
    cs.append(Case("two_large", [two(B + 3), two(2 * S + 5) + 1], 9))
    cs.append(Case("large_then_step", [two(3 * S)] + small(rng, [2] * 30, 9), 9))
    cs.append(Case("empty_front", [[], [], []] + small(rng, [4, 5, 6], 9), 9))
    cs.append(Case("empty_end", small(rng, [4, 5, 6], 9) + [[], [], []], 9))
    cs.append(Case("empty_runs", [[]] * 5 + small(rng, [2], 9) + [[]] * (SD + 3) + small(rng, [3], 9) + [[]] * 2, 9))
    cs.append(Case("empty_batch", [[]] * 17, 9))
    cs.append(Case("empty_batch_long", [[]] * (2 * SD + 1), 9))
    cs.append(Case("no_docs", [], 9))
    cs.append(Case("no_terms", [[], []], 0))
    cs.append(Case("off0", small(rng, [4, 0, 9, 3], 9), 9, lead=13))
    cs.append(Case("cut_middle", small(rng, [6] * 300, 31), 31, lead=777, tail=99))
    cs.append(Case("one_doc", [[2, 2, 5]], 9))
    cs.append(Case("one_entry", [[0]], 1))
    cs.append(Case("step_docs", small(rng, [1] * (SD + 1), 5) + small(rng, [0, 1] * SD, 5), 5))
    # several workgroups: small documents up to just below a range's weight, a large document on the border, then more
    k = (RW - 20) // 8
    cs.append(Case("ranges", small(rng, [7] * k, 29) + [two(B + 5)] + small(rng, [7] * (4 * k), 29), 29))
    cs.append(Case("ranges_lines", small(rng, rng.integers(0, 4, 6 * RW // 2), 301), 301))
    cs.append(Case("hot_term", [[3] * 9] * 700, 5))
    cs.append(Case("cache_collide", [[7, 7 + CS, 7, 7 + CS]] * (3 * S // 4), 2 * CS + 9))
    cs.append(Case("cache_triple", [[7, 7 + CS, 7 + 2 * CS, 7, 7 + CS, 7 + 2 * CS]] * (S // 2), 3 * CS))
    cs.append(Case("cache_evict", [np.arange(i * 8, i * 8 + 8) for i in range(3 * S // 8)], 3 * S + 1))
    cs.append(Case("cache_evict_large", [np.arange(3 * S + 9)], 3 * S + 9))
    cs.append(Case("set_collide", [[5, 5 + SS, 5 + 2 * SS, 5, 5 + SS]] * 150 + [[5 + SS, 5]] * 150, 3 * SS))
    cs.append(Case("one_term", small(rng, [3, 0, 5, 1] * 50, 1), 1))
    cs.append(Case("one_term_large", [[0] * (B + 1)], 1))
    for nt in (LT - 1, LT, LT + 1, LT + 70):
        d = two(B + 9).copy()
        d[5::7] = nt - 1                                            # the highest term id, again and again
        cs.append(Case("bitset_%d" % nt, small(rng, [3, 3], nt) + [d] + [[nt - 1, 0, nt - 1]], nt))
    return cs


def random_cases(sh, n, seed=7):
    S = sh["step_entries"]
    out = []
    for i in range(n):
        rng = np.random.default_rng(seed * 1000 + i)
        n_terms = int(rng.choice([3, 50, 1000, 5000, sh["cache_slots"] * 4 + 3]))
        kind = i % 4
        if kind == 0:
            docs = zipf_docs(rng, int(rng.integers(1, 900)), n_terms, 4.0)
        elif kind == 1:
            docs = zipf_docs(rng, int(rng.integers(1, 12)), n_terms, S * 0.6)
        elif kind == 2:
            docs = zipf_docs(rng, 200, n_terms, 2.0) + zipf_docs(rng, 2, n_terms, 1.5 * S) + zipf_docs(rng, 300, n_terms, 6.0)
        else:
            docs = zipf_docs(rng, int(rng.integers(1, 3000)), n_terms, 0.7)
        out.append(Case("random_%d" % i, docs, n_terms, lead=int(rng.integers(0, 50)), tail=int(rng.integers(0, 50))))
    return out


def fresh(n_terms, pattern=None):
    if pattern is None:
        return np.zeros(n_terms, np.uint64), np.zeros(n_terms, np.uint64), np.zeros(n_terms, np.uint64)
    return tuple(np.full(n_terms, pattern + k, np.uint64) for k in range(3))


def check_case(run, case, doc_base=0):
    """overwrite mode into arrays that hold a pattern: every entry is written"""
    occ, docs, first = fresh(case.n_terms, 0x1111111111111111)
    assert run(case.off, case.term, case.n_docs, case.n_terms, 0, doc_base, occ, docs, first) == 0, case.name
    want = reference(case.off, case.term, case.n_docs, case.n_terms, doc_base)
    for name, g, w in zip(("occ", "docs", "first"), (occ, docs, first), want):
        bad = np.nonzero(g != w)[0]
        assert not bad.size, "%s: %s[%d] = %d, expected %d (%d differ)" % (case.name, name, bad[0], g[bad[0]], w[bad[0]], bad.size)


def check_null_outputs(run, case):
    want = reference(case.off, case.term, case.n_docs, case.n_terms, 5)
    for k in range(3):
        arrs = list(fresh(case.n_terms, 0x2222222222222222))
        keep = [a.copy() for a in arrs]
        args = [a if j != k else None for j, a in enumerate(arrs)]
        assert run(case.off, case.term, case.n_docs, case.n_terms, 0, 5, *args) == 0
        for j in range(3):
            assert (arrs[j] == (keep[j] if j == k else want[j])).all(), (case.name, k, j)
    assert run(case.off, case.term, case.n_docs, case.n_terms, 0, 5, None, None, None) == 0


def check_accumulate_halves(run, case, cut_doc):
    """two calls over two halves (cut at a document border) equal one call over the whole"""
    n, nt = case.n_docs, case.n_terms
    occ, docs, first = fresh(nt)
    first[:] = MAX
    assert run(case.off[:cut_doc + 1], case.term, cut_doc, nt, ACC, 100, occ, docs, first) == 0
    assert run(case.off[cut_doc:], case.term, n - cut_doc, nt, ACC, 100 + cut_doc, occ, docs, first) == 0
    w_occ, w_first = reference(case.off, case.term, n, nt, 100)[0::2]
    assert (occ == w_occ).all() and (first == w_first).all(), case.name
    # a term counts once per document and half: the sum of the halves' document frequencies
    d1 = reference(case.off[:cut_doc + 1], case.term, cut_doc, nt)[1]
    d2 = reference(case.off[cut_doc:], case.term, n - cut_doc, nt)[1]
    assert (docs == d1 + d2).all() and (docs == reference(case.off, case.term, n, nt)[1]).all(), case.name


def check_accumulate_carry(run):
    """a counter that stands at 2^32 - 1 carries into bit 32; first keeps the smaller of what it holds and the batch's"""
    c = Case("carry", [[2, 2, 1], [], [2, 3]], 6)
    occ, docs, first = (np.full(6, 0xFFFFFFFF, np.uint64) for _ in range(3))
    first[:] = [0, 3, 1000, 1001, 7, MAX]                           # below, below, above, equal-to, untouched, none
    assert run(c.off, c.term, 3, 6, ACC, 1000, occ, docs, first) == 0
    assert occ.tolist() == [0xFFFFFFFF, 1 << 32, (1 << 32) + 2, 1 << 32, 0xFFFFFFFF, 0xFFFFFFFF]
    assert docs.tolist() == [0xFFFFFFFF, 1 << 32, (1 << 32) + 1, 1 << 32, 0xFFFFFFFF, 0xFFFFFFFF]
    assert first.tolist() == [0, 3, 1000, 1001, 7, int(MAX)]
    first[:] = [0, 2000, 999, 1003, 7, MAX]
    assert run(c.off, c.term, 3, 6, ACC, 1000, occ, docs, first) == 0
    assert first.tolist() == [0, 1000, 999, 1002, 7, int(MAX)]
    assert occ[2] == (1 << 32) + 5


def refusal_inputs(sh):
    """(name, off, term, n_docs, n_terms, flags): every one is GFT_E_INVALID"""
    S = sh["step_entries"]
    rng = np.random.default_rng(3)
    base = Case("base", small(rng, [5] * (S // 2), 40), 40)
    out = []
    t = base.term.copy(); t[len(t) // 2] = 40
    out.append(("term_eq_n_terms", base.off, t, base.n_docs, 40, 0))
    t = base.term.copy(); t[0] = 0xFFFFFFFF
    out.append(("term_max_first", base.off, t, base.n_docs, 40, 0))
    t = base.term.copy(); t[-1] = 0xFFFFFFFF
    out.append(("term_max_last", base.off, t, base.n_docs, 40, ACC))
    o = base.off.copy(); o[base.n_docs // 2] -= np.uint64(7)
    out.append(("offset_descends", o, base.term, base.n_docs, 40, 0))
    o = base.off.copy(); o[-1] = 0; o[0] = 5
    out.append(("ends_descend", o, base.term, base.n_docs, 40, 0))
    out.append(("unknown_flags", base.off, base.term, base.n_docs, 40, 2))
    out.append(("unknown_flags_high", base.off, base.term, base.n_docs, 40, ACC | 0x80000000))
    out.append(("entries_no_terms", base.off, base.term, base.n_docs, 0, 0))
    return out


def check_refusal(run, off, term, n_docs, n_terms, flags):
    nt = max(n_terms, 40)
    arrs = fresh(nt, 0x5A5A5A5A5A5A5A00)
    keep = [a.copy() for a in arrs]
    assert run(off, term, n_docs, n_terms, flags, 9, *arrs) == E_INVALID
    for a, k in zip(arrs, keep):
        assert a.tobytes() == k.tobytes(), "a refused call wrote"


# ---- columns ------------------------------------------------------------------------------------------------------------------

def columns_reference(bitmap, n_cols, row_idx=None):
    W = (n_cols + 31) // 32
    bm = np.asarray(bitmap, dtype=np.uint32).reshape(-1, W) if W else np.zeros((0, 0), np.uint32)
    rows = bm if row_idx is None else bm[np.asarray(row_idx, dtype=np.int64)]
    bits = (rows[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]) & 1
    return bits.reshape(rows.shape[0], W * 32)[:, :n_cols].sum(axis=0).astype(np.uint64)


def column_cases(sh):
    """(name, bitmap [n, W] with garbage above n_cols, n_cols, row_idx or None)"""
    R = sh["column_rows"]
    rng = np.random.default_rng(11)
    out = []
    for n_cols in (1, 31, 32, 33, 65):
        for n_rows in (0, 1, 63, 64, 65, 2 * R + 77):
            W = (n_cols + 31) // 32
            bm = rng.integers(0, 1 << 32, (n_rows, W), dtype=np.uint64).astype(np.uint32)
            bm &= rng.integers(0, 1 << 32, (n_rows, W), dtype=np.uint64).astype(np.uint32)       # (a quarter of the bits)
            out.append(("cols%d_rows%d" % (n_cols, n_rows), bm, n_cols, None))
    bm = rng.integers(0, 1 << 32, (300, 3), dtype=np.uint64).astype(np.uint32)
    out.append(("row_idx_repeats", bm, 70, np.array([5, 5, 5, 299, 0, 0, 17] * 40, dtype=np.uint64)))
    out.append(("row_idx_long", bm, 70, rng.integers(0, 300, R + 300).astype(np.uint64)))
    out.append(("row_idx_empty", bm, 70, np.zeros(0, dtype=np.uint64)))
    out.append(("all_set", np.full((R + 1, 2), 0xFFFFFFFF, np.uint32), 40, None))
    return out


def check_columns(run_cols, name, bm, n_cols, row_idx):
    n_rows = len(row_idx) if row_idx is not None else bm.shape[0]
    want = columns_reference(bm, n_cols, row_idx)
    count = np.full(n_cols, 0x3333333333333333, np.uint64)
    assert run_cols(bm, n_rows, n_cols, row_idx, 0, count) == 0, name
    assert (count == want).all(), name
    count[:] = 0xFFFFFFFF
    assert run_cols(bm, n_rows, n_cols, row_idx, ACC, count) == 0, name
    assert (count == want + np.uint64(0xFFFFFFFF)).all(), name      # (64-bit: the carry into bit 32)
    keep = count.copy()
    assert run_cols(bm, n_rows, n_cols, row_idx, 4, count) == E_INVALID and (count == keep).all(), name
