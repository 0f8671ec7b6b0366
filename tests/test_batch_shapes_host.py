"""The generators of batch_shapes.py on the CPU: what test_gpu_batch_shapes.py relies on, so that it cannot pass vacuously.
A: the expansion of the per-pool-string expectations IS the oracle's answer over the whole batch of N documents, and every
prefix sum the device computes for that batch has something to carry across item 2^20.  B: the oracle counts exactly the
constructed number of matches in every document, every listed count and layout is there, and the oracle agrees with its
brute-force enumerator."""
import numpy as np
import pytest

import batch_shapes as S
from helpers import assert_csr_equal
from oracle.pyoracle import Oracle, POS_END, POS_START
from test_table_set import tables

_CACHE = {}


def expected():
    if "x" not in _CACHE:
        _CACHE["x"] = S.Expected()
    return _CACHE["x"]


def index_array(variant):
    if variant not in _CACHE:
        _CACHE[variant] = S.index_array(variant)
    return _CACHE[variant]


VARIANTS = pytest.mark.parametrize("variant", ["full", "holes"])


def test_pool_holds_every_kind_of_document():
    x = expected()
    p = x.pool
    assert len(p) <= 64 and len(set(p)) == len(p) and p[-1] == b"" and all(1 <= len(s) <= 12 for s in p[:-1])
    assert len(S.TERMS_A) == 10 and all(1 <= len(t) <= 5 for t in S.TERMS_A)
    n = [len(t) for t, _ in x.csr[POS_START]]
    assert n.count(0) >= 5 and n.count(1) >= 3 and max(n) >= 6
    assert any(len(t) > len(set(t.tolist())) for t, _ in x.csr[POS_START]), "no document repeats a term"
    # rune offsets differ from byte offsets behind a 2-byte and behind a 3-byte rune
    shifts = {int(b) - int(r) for (_, pp), rr in zip(x.csr[POS_START], x.rune_rows) for b, r in zip(pp, rr)}
    assert {0, 1, 2, 3} <= shifts
    changed = [len(lo) - len(s) for s, lo in zip(p, x.lower_rows) if lo != s]
    assert any(c < 0 for c in changed) and any(c > 0 for c in changed) and changed.count(0) >= 3
    assert "Éab".encode() in p and any(b"\xff" in s for s in p)


@VARIANTS
def test_batch_has_the_stated_shape(variant):
    x, idx = expected(), index_array(variant)
    assert idx.size == S.N_BIG == 1_052_673 and (S.N_BIG + S.SCAN_TILE - 1) // S.SCAN_TILE == 258
    blob, off = x.text(idx)
    lens = np.diff(off.astype(np.int64))
    assert off[0] == 0 and off[-1] == blob.size and 5_000_000 < blob.size * (1.5 if variant == "holes" else 1) < 9_000_000
    if variant == "full":
        assert lens.min() >= 1
        assert int(x.rune_blocks(idx).sum()) > S.BORDER
    else:
        assert 0.3 < (lens == 0).mean() < 0.37 and not lens[list(S.EDGE_DOCS)].any()
    assert np.unique(idx).size == len(x.pool) - (variant == "full")      # every pool string is drawn


@VARIANTS
@pytest.mark.parametrize("mode", S.POS_MODES, ids=["start", "end"])
def test_expansion_is_the_oracle_over_the_whole_batch(variant, mode):
    x, idx = expected(), index_array(variant)
    blob, off = x.text(idx)
    assert_csr_equal(x.scan(idx, mode), Oracle(S.TERMS_A, mode).scan(blob, off))


@VARIANTS
def test_bitmap_expansion_is_the_oracle_and_every_expression_has_both_values(variant):
    x, idx = expected(), index_array(variant)
    blob, off = x.text(idx)
    o = Oracle(S.TERMS_A, POS_START)
    o.set_expressions(S.EXPRS_A, True)
    bm = x.bitmap(idx)
    assert np.array_equal(bm, o.process(blob, off))
    for e in range(len(S.EXPRS_A)):
        share = float((bm[:, e >> 5] >> (e & 31) & 1).mean())
        assert 0.1 <= share <= 0.9, (S.EXPRS_A[e], share)


def test_long_document_variant_is_the_oracle_too():
    x, idx = expected(), index_array("full")
    blob, off = S.with_long_document(*x.text(idx), S.BORDER)
    assert int(off[S.BORDER + 1] - off[S.BORDER]) == S.LONG_DOC_LEN > S.UNIT_MAX and off[-1] == blob.size
    o = Oracle(S.TERMS_A, POS_START)
    o.set_expressions(S.EXPRS_A, True)
    want = x.bitmap(idx)
    want[S.BORDER] = o.process(np.frombuffer(S.long_document(), np.uint8), np.asarray([0, S.LONG_DOC_LEN], np.uint64))[0]
    assert np.array_equal(want, o.process(blob, off))
    assert int(want[S.BORDER, 0]) != int(x.bitmap(idx)[S.BORDER, 0])


@VARIANTS
def test_every_prefix_sum_crosses_the_border_with_something_to_carry(variant):
    """the inputs of the device's scans over documents: work units, matches, unique terms, rune blocks, lower-case lengths
    and true expressions per document -- non-zero on both sides of item 2^20, and (full batch) non-zero in the two documents
    next to the border, so that the running sums at 1 048 575, 1 048 576 and 1 048 577 all differ"""
    x, idx = expected(), index_array(variant)
    bm = x.bitmap(idx)
    sums = {"matches": np.diff(x.scan(idx, POS_START)[0].astype(np.int64)),
            "unique terms": np.diff(x.unique(idx)[0].astype(np.int64)),
            "rune blocks": x.rune_blocks(idx),
            "lower-case bytes": np.diff(x.lower(idx)[1].astype(np.int64)),
            "true expressions": sum((bm[:, 0] >> e & 1).astype(np.int64) for e in range(len(S.EXPRS_A)))}
    for name, c in sums.items():
        assert c.size == S.N_BIG
        assert c[:S.BORDER].sum() > 0 and c[S.BORDER:].sum() > 0 and c[S.BORDER + 1:].sum() > 0, name
        assert c[S.SCAN_TILE:].sum() > 0 and c[:S.SCAN_TILE].sum() > 0, name
        if variant == "full":
            assert c[S.BORDER - 1] > 0 and c[S.BORDER] > 0 and c[S.SCAN_TILE - 1] > 0 and c[S.SCAN_TILE] > 0 and c[-1] > 0, name
        elif name != "true expressions":                 # (a NOT is true of an empty document)
            assert not c[list(S.EDGE_DOCS)].any() and (c == 0).mean() > 0.3, name
    # the matches themselves are more than 2^20 items as well (the units' slabs, the rune mapping's search)
    assert sums["matches"].sum() > S.BORDER and sums["unique terms"].sum() > S.BORDER


def test_unique_and_rune_expansions_follow_from_the_scan():
    x = expected()
    idx = np.arange(len(x.pool))
    mo, ti, po = x.scan(idx, POS_START)
    uo, ut, up = x.unique(idx)
    ro, rt, rp = x.runes(idx)
    assert np.array_equal(ro, mo) and np.array_equal(rt, ti) and not up.any()
    for d, s in enumerate(x.pool):
        a, b = int(mo[d]), int(mo[d + 1])
        assert ut[int(uo[d]):int(uo[d + 1])].tolist() == list(dict.fromkeys(ti[a:b].tolist()))
        assert rp[a:b].tolist() == [len(s[:int(q)].decode("utf-8", "replace")) for q in po[a:b]], s


# ---- B ------------------------------------------------------------------------------------------------------------------------
FAMILY_NAMES = sorted(S.FAMILIES)


@pytest.mark.parametrize("mode", S.POS_MODES, ids=["start", "end"])
@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_oracle_counts_are_the_constructed_ones(name, mode):
    fam = S.FAMILIES[name]()
    blob, off = fam.packed()
    o = fam.oracle(mode)
    csr = o.scan(blob, off)
    assert np.diff(csr[0].astype(np.int64)).tolist() == fam.counts
    assert_csr_equal(csr, o.brute(blob, off))
    uo, ut, up = fam.unique_of(csr)
    # (longer runs reach longer terms: a document's distinct terms are min(longest run, kmax) and `b`)
    assert np.diff(uo.astype(np.int64)).tolist() == [min(max(map(len, t.replace(b"b", b"x").split(b"x"))), fam.kmax) + (b"b" in t) for t in fam.texts]
    assert not up.any() and ut.size == int(uo[-1])


def test_every_listed_count_and_layout_occurs():
    ex = S.family_exact()
    by_count = {}
    for t, c in zip(ex.texts, ex.counts):
        by_count.setdefault(c, []).append(len(t))
    for c in S.EXACT_COUNTS:
        lens = by_count[c]
        assert S.UNIT_MAX in lens and min(lens) == (c + 1) // 2 + (c + 1) % 2, c       # embedded, and the shortest form
        assert min(lens) <= 256 or c > 511
    assert {len(t) for t in ex.texts} >= set(S.UNIT_LENGTHS) | {8193, 16385}
    for t in ex.texts:
        if len(t) in S.UNIT_LENGTHS and t[1:2] == b"b":
            assert t[0] == 0x61 and t[-1] == 0x61                                    # matches end at the first and at the last byte
    assert ex.texts.count(b"") >= 10 and all(len(t) <= S.UNIT_MAX or len(t) in (8193, 16385) for t in ex.texts)
    # the cut documents: unit borders (as k_unit_fill cuts them) inside a run of `a`
    for n, k in ((8193, 2), (16385, 3)):
        t = next(t for t in ex.texts if len(t) == n)
        per = (n + k - 1) // k
        assert per <= S.UNIT_MAX and all(t[i * per - 1:i * per + 1] == b"aa" for i in range(1, k))
    ob = S.family_onebin()
    assert sorted(set(ob.counts)) == [0, 255, 256, 257]
    for t, c in zip(ob.texts, ob.counts):
        if len(t) == S.UNIT_MAX:
            ends = [i for i, ch in enumerate(t) if ch != 0x78]
            assert len({e >> 5 for e in ends}) in (1, 2)                             # (bins of 32 end offsets: shift 5)
    one = [c for t, c in zip(ob.texts, ob.counts) if len(t) == S.UNIT_MAX and len({i >> 5 for i, ch in enumerate(t) if ch != 0x78}) == 1]
    two = [c for t, c in zip(ob.texts, ob.counts) if len(t) == S.UNIT_MAX and len({i >> 5 for i, ch in enumerate(t) if ch != 0x78}) == 2]
    assert sorted(set(one)) == sorted(set(two)) == [255, 256, 257]
    ti = S.family_ties()
    assert {2464, 253} <= set(ti.counts) and max(S.family_ties200().counts) == 31300 == 200 * 256 - 19900
    assert (31300 + S.FIFO - 1) // S.FIFO == 123
    il = S.family_interleave()
    assert sum(1 for t in il.texts if t) == S.INTERLEAVE_DOCS > S.GATHER_WAVES_PER_CU * 256
    assert {0, 1, 6, 255, 256, 259} == set(il.counts)


def test_every_dictionary_gets_the_kernel_it_is_tested_on():
    """plan_scan for gfx950, without a device: unforced, part A and every family run scan5, whose slabs go through
    k_gather_sorted, as scan3's do; forced, each dictionary gets the kernel the GPU module asks for"""
    for terms in [list(S.TERMS_A)] + [list(f().terms) for f in S.FAMILIES.values()]:
        assert [tables(terms, forced=k)[0] for k in ("auto", "scan5", "scan3", "dfa")] == ["scan5", "scan5", "scan3", "dfa"]
