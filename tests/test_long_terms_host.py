"""Keywords of 301 to 7 424 bytes on the CPU (no GPU): the families of tests/long_terms.py are what they claim to be, the
oracle agrees at these lengths with a brute-force match list that knows no automaton (bytes.find per keyword and document),
and plan_scan / the table blob at the longest keyword gft_build accepts.  tests/test_gpu_long_terms.py runs the same
families through the kernels and compares with the oracle -- which this file makes trustworthy there."""
import ctypes as C

import numpy as np
import pytest

import long_terms as lt
from gofindthem_amd import _lib
from helpers import Refused, assert_csr_equal, learned_unit, scan_plan, tables, tree_to_program
from oracle import dsl_ref
from oracle.pyoracle import Oracle, POS_END, POS_START, pack_strings


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for name in ("GFT_SCAN_KERNEL", "GFT_SCAN5_LARGE", "GFT_SCAN5_GROUPS", "GFT_SCAN5_BLOOM_KB", "GFT_SCAN5_FIFO"):
        monkeypatch.delenv(name, raising=False)


def long_ids(terms):
    return {i for i, t in enumerate(sorted(set(terms))) if len(t) > 300}


@pytest.mark.parametrize("L", lt.LENGTHS)
@pytest.mark.parametrize("name", lt.FAMILIES)
def test_oracle_is_the_brute_force_list(name, L):
    terms, docs, fold = lt.family(name, L)
    assert max(len(t) for t in terms) == L and min(len(t) for t in terms) <= 4
    assert all(len(d) <= lt.DOC_MAX for d in docs) and sum(len(d) for d in docs) <= 200_000
    blob, off = pack_strings(docs)
    ids = long_ids(terms)
    for pos_mode in lt.POS_MODES:
        want = lt.brute_force(terms, docs, pos_mode, fold)
        got = Oracle(terms, pos_mode).scan(blob, off, fold=fold)
        assert_csr_equal(got, want)
        assert_csr_equal(lt.expected(name, L, pos_mode), want)
        n_long = int(np.isin(want[1], list(ids)).sum())
        assert want[1].size < 1_000_000
        if name == "near_misses":
            assert n_long == 0 and want[1].size > 0
        else:
            assert n_long > 0
    # dense enough for `learn` to take the suffix-window kernels' units down to 512 bytes after one call (periodic and
    # planted are scanned twice on the GPU for that): more than 0.25 matches per byte at the planned fifo of 256 entries
    if name in ("planted", "periodic", "folded"):
        kernel, plan = scan_plan(terms)
        assert kernel == "scan5" and learned_unit(kernel, plan["fifo_cap"], int(want[1].size), 0, int(off[-1])) == 512


@pytest.mark.parametrize("L", lt.LENGTHS)
def test_planted_keywords_lie_where_the_builder_says(L):
    """byte 0 of the first document, a whole document, the blob's last byte, the last two bytes of a unit and the first two of
    the next at the slices of 507, 1 000 and 8 000 bytes, and matches that start in one 507-byte unit and end 1, 7, 14 later:
    each placement is in the brute-force list of its document"""
    for letters in (False, True):
        terms, docs, layout = lt.planted_layout(L, letters)
        moff, tid, pos = lt.brute_force(terms, docs, POS_START)
        ids = {t: i for i, t in enumerate(sorted(set(terms)))}
        per_doc = [set(zip(tid[int(moff[d]):int(moff[d + 1])].tolist(), pos[int(moff[d]):int(moff[d + 1])].tolist())) for d in range(len(docs))]
        whats = set()
        for d, start, kw, what in layout:
            assert (ids[kw], start) in per_doc[d], what
            end = start + len(kw) - 1
            whats.add(what)
            if what.startswith("ends at byte"):
                r, per = int(what.split()[3]), int(what.split()[6].split("-")[0])
                assert len(docs[d]) == lt.DOC_MAX and end % per == r and per in [lt.unit_slice(lt.DOC_MAX, u) for u in lt.UNIT_SIZES]
            elif what.startswith("starts on a unit's last byte"):
                j = int(what.split()[-3])
                assert len(docs[d]) == lt.DOC_MAX and end // lt.SPAN_UNIT - start // lt.SPAN_UNIT == j
        K = terms[len(lt.SHORT)]
        assert len(K) == L and docs[0].startswith(K) and docs[-1].endswith(K) and K in docs and docs[1] == b""
        u = lt.TEXT_BUF - (L - 1)
        fills = [d for d, _, _, what in layout if "fills kTextBuf" in what]
        assert len(whats) == 3 + 12 + sum(1 for j in lt.SPANS if j * lt.SPAN_UNIT + 1 < L) + len(fills)
        if L >= 7423:
            # k_scan_units: nbytes = unit + warm-up reaches kTextBuf exactly, in the units 8 and 9 of a ten-unit document
            assert len(fills) == 1 and len(docs[fills[0]]) == 10 * u and lt.unit_slice(10 * u, u) == u
            assert u + (L - 1) == lt.TEXT_BUF == 8448 and 8 * u >= L - 1
        else:
            assert not fills
        assert any(lt.E_ACUTE in d for d in docs) is letters
    assert [lt.unit_slice(lt.DOC_MAX, u) for u in lt.UNIT_SIZES] == [507, 1000, 8000]
    # the longest keyword reaches back over fourteen and more units of 512 bytes
    if L == lt.MAX_LEN:
        assert (L - 1) // lt.SPAN_UNIT == 14


def test_folded_text_needs_the_fold():
    terms, docs, fold = lt.family("folded", 513)
    assert fold and any(d != d.lower() for d in docs)
    plain = lt.brute_force(terms, docs, POS_START, fold=False)
    ids = long_ids(terms)
    assert not np.isin(plain[1], list(ids)).any()


# ---- the solver scenario -------------------------------------------------------------------------------------------------
def _bit(bm, d, e):
    return bool(bm[d, e >> 5] >> (e & 31) & 1)


def test_solver_scenario_depends_on_the_long_match():
    """the oracle's answers on the scenario's documents: with L (or M) intact the first group is true with `y` at 300 alone
    (start positions: the first L-or-s behind x is 11), with the keyword broken it is false (... is 600) and true again with a
    `y` at 8 000; in end-position mode the two placements of `y` give different bits for the intact keyword.  The brute-force
    list agrees with the oracle's scan on these documents."""
    c = lt.solver_case()
    docs, names, exprs = c["docs"], c["names"], c["exprs"]
    blob, off = pack_strings(docs)
    at = {n: i for i, n in enumerate(names)}
    for pos_mode in lt.POS_MODES:
        o = Oracle(c["terms"], pos_mode)
        assert_csr_equal(o.scan(blob, off), lt.brute_force(c["terms"], docs, pos_mode))
        o.set_expressions(exprs, True)
        bm = o.process(blob, off)
        for k, g0 in (("a", 0), ("m", 4)):
            first, chain = g0, g0 + 1
            if pos_mode == POS_START:
                assert _bit(bm, at[k], first) and _bit(bm, at[k + "_late"], first)
                assert not _bit(bm, at[k + "_broken"], first) and _bit(bm, at[k + "_broken_late"], first)
                assert _bit(bm, at[k], chain) and not _bit(bm, at[k + "_broken"], chain)
            else:
                assert not _bit(bm, at[k], first) and _bit(bm, at[k + "_late"], first)
                assert not _bit(bm, at[k], chain) and _bit(bm, at[k + "_late"], chain)
                assert not _bit(bm, at[k + "_broken_late"], chain)
            for g in range(c["n_groups"]):                                       # the NOT forms are the complements
                for d in range(len(docs)):
                    assert _bit(bm, d, g) != _bit(bm, d, g + c["n_groups"])
    # the geometry the scenario is about: at 512-byte units the documents are 8 units or more, L ends 14 units behind `s`
    per = lt.unit_slice(lt.SOLVER_DOC, 512)
    assert lt.SOLVER_DOC // per >= 8 and (lt.L_AT + lt.MAX_LEN - 1) // per - lt.S_IN // per >= 13
    assert all(len(d) >= 6000 for d in docs) and all(len(d) <= lt.DOC_MAX for d in docs)
    a = docs[at["a"]]
    assert a[lt.X_AT:lt.L_AT] == lt.X and a.find(c["L"]) == lt.L_AT and a.find(lt.Y) == lt.Y_IN and a.count(lt.Y) == 1
    assert a.find(lt.S_) == lt.S_IN and a.find(lt.S_, lt.S_IN + 1) == lt.S_LATE
    assert docs[at["a_late"]].find(lt.Y, lt.Y_IN + 1) == lt.Y_LATE and docs[at["a_broken"]].find(c["L"]) < 0


def _succ_min_by_units(term, pos, ends, per, n_units, queries, back):
    """wave_succ_min's walk of a document of 8 units or more (csrc/gft_solve.hip), restated: a unit holds the matches that END in
    its slice; start at the slice of the smallest threshold, four units a step, stop when the next slice begins more than `back`
    bytes behind the best answer so far.  queries = [(slot, theta)] -> the smallest position > theta of its slot, or None"""
    unit_of = ends // per
    ub, best = min(th for _, th in queries) // per if min(th for _, th in queries) >= 0 else 0, None
    ub = min(ub, n_units - 1)
    while ub < n_units:
        if best is not None and ub * per - back > best:
            break
        here = (unit_of >= ub) & (unit_of < ub + 4)
        for slot, th in queries:
            hit = pos[here & (term == slot) & (pos > th)]
            if hit.size and (best is None or int(hit.min()) < best):
                best = int(hit.min())
        ub += 4
    return best


def test_early_stop_of_the_unit_walk_needs_the_look_back():
    """the scenario is one that a walk which ignored max_term_len would answer wrongly: over the oracle's matches of document
    `a`, cut into 500-byte units by where they end, "the first L or s behind x" is 11 with back = 7 423 and 600 with back = 0
    (the 7 424-byte match lies in unit 14, the walk would have stopped behind units 0-3) -- so the expected bit of
    test_gpu_long_terms.py::test_inord_groups_over_a_7424_byte_match is one that such a kernel gets wrong"""
    c = lt.solver_case()
    dictionary = sorted(set(c["terms"]))
    text = c["docs"][c["names"].index("a")]
    blob, off = pack_strings([text])
    _, tid, pos = Oracle(c["terms"], POS_START).scan(blob, off)
    lens = np.asarray([len(t) for t in dictionary])
    pos = pos.astype(np.int64)
    ends = pos + lens[tid] - 1
    per = lt.unit_slice(len(text), 512)
    n_units = (len(text) + per - 1) // per
    assert n_units >= 8
    queries = [(dictionary.index(c["L"]), lt.X_AT), (dictionary.index(lt.S_), lt.X_AT)]
    assert _succ_min_by_units(tid, pos, ends, per, n_units, queries, back=lt.MAX_LEN - 1) == lt.L_AT
    assert _succ_min_by_units(tid, pos, ends, per, n_units, queries, back=0) == lt.S_IN
    assert int(ends[tid == queries[0][0]][0]) // per - lt.S_IN // per == 13


def test_host_solver_on_the_scenario():
    """the product's host solver (gft_debug_host_solve: what gft_process* runs for pairs the device does not answer) on the
    scenario's position lists against the oracle"""
    c = lt.solver_case()
    L = _lib.load()
    docs, exprs = c["docs"] + lt.solver_short_docs(), c["exprs"]
    blob, off = pack_strings(docs)
    dictionary = sorted(set(c["terms"]))
    for pos_mode in lt.POS_MODES:
        o = Oracle(c["terms"], pos_mode)
        o.set_expressions(exprs, True)
        want = o.process(blob, off)
        moff, tid, pos = o.scan(blob, off)
        progs = [np.asarray(tree_to_program(dsl_ref.parse(e, True)[0], lambda lit: dictionary.index(lit.encode())), np.uint32) for e in exprs]
        for d in range(len(docs)):
            t, p = tid[int(moff[d]):int(moff[d + 1])], pos[int(moff[d]):int(moff[d + 1])]
            slots = np.unique(t).astype(np.uint32)
            lists = [np.sort(p[t == s]).astype(np.int64) for s in slots]
            lo = np.zeros(len(lists) + 1, np.uint64)
            if lists:
                lo[1:] = np.cumsum([x.size for x in lists])
            flat = np.concatenate(lists) if lists else np.zeros(1, np.int64)
            for e, w in enumerate(progs):
                out = C.c_int(-1)
                assert L.gft_debug_host_solve(w.ctypes.data, w.size, slots.ctypes.data if slots.size else None, lo.ctypes.data,
                                              flat.ctypes.data, len(lists), C.byref(out)) == 0
                assert bool(out.value) == _bit(want, d, e), (pos_mode, d, exprs[e][:40])


# ---- plan boundary -------------------------------------------------------------------------------------------------------
def test_plan_at_the_longest_accepted_keyword():
    """plan_scan for a dictionary whose longest keyword is 7 424 bytes: scan5 by default, a fifo entry of term id (as many bits
    as the dictionary needs) and a position relative to unit.lo - (7 424 + kScan2MaxOff), which must fit the other bits next to
    a unit of 8 192 bytes; scan3 and dfa when forced; 7 425 is refused by every route"""
    for name in ("planted", "shared_suffix", "periodic"):
        terms = lt.family(name, lt.MAX_LEN)[0]
        kernel, p = scan_plan(terms)
        n = len(set(terms))
        bits = max(1, (n - 1).bit_length())
        assert kernel == "scan5" and tables(terms)[0] == "scan5"
        assert p == dict(max_term_len=7424, s5_term_bits=bits, s5_pos_bias=7428, fifo_cap=p["fifo_cap"]) and 64 <= p["fifo_cap"] <= 512
        assert 8192 + p["s5_pos_bias"] + 8 < 1 << (32 - p["s5_term_bits"])
        for forced in ("scan3", "dfa"):
            assert scan_plan(terms, forced)[0] == forced and tables(terms, forced=forced)[0] == forced
            assert scan_plan(terms, forced)[1]["s5_pos_bias"] == 0
    terms = lt.family("planted", 7423)[0]
    assert scan_plan(terms)[1]["s5_pos_bias"] == 7427
    too_long = lt.SHORT + [b"abcdefgh" * 928 + b"a"]
    assert len(too_long[-1]) == 7425
    with pytest.raises(Refused):
        scan_plan(too_long)
    with pytest.raises(Refused, match="keyword longer than 7424 bytes"):
        tables(too_long)


@pytest.mark.parametrize("name", ["planted", "shared_suffix"])
def test_blob_of_a_7424_byte_dictionary_round_trips(name):
    """gft_export_tables' writer and gft_import_tables' reader on such a dictionary: byte for byte, same kernel"""
    terms = lt.family(name, lt.MAX_LEN)[0]
    for forced in ("auto", "scan3", "dfa"):
        kernel, blob = tables(terms, forced=forced)
        kernel2, blob2 = tables(blob=blob, forced=forced)
        assert blob2 == blob and kernel2 == kernel
