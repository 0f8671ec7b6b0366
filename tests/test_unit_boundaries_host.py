"""The batches of tests/unit_boundaries.py are what they claim (no GPU): every length and every pair of length classes, the
document at blob offset 0 behind the run of empty ones, text across doc_off[0] and the blob's end that completes keywords,
keywords across every unit border of the long document at both unit sizes, a density that teaches 512-byte units with and without
positions, units that outgrow the fifo -- and the oracle's answers are not trivial."""
import numpy as np
import pytest

import unit_boundaries as ub
from helpers import learned_unit, scan_plan
from long_terms import brute_force
from oracle.pyoracle import POS_START, pack_strings
from presence_once import Model

KERNEL, PLAN = scan_plan(ub.TERMS)
FIFO_CAP = PLAN["fifo_cap"]


def test_names_and_sizes():
    c = ub.cases()
    assert sorted(c) == sorted(["pairs", "blob_end", "long_doc", "second_walk"] + ["empty_run_lead%d" % n for n in ub.LEADS])
    assert KERNEL == "scan5"
    assert 60 <= len(ub.TERMS) <= 80 and min(map(len, ub.TERMS)) == 1 and max(map(len, ub.TERMS)) == 300
    for name, case in c.items():
        if name != "pairs":
            assert 40 <= len(case.docs) <= 70, name          # documents; sixteen waves have a next unit several times
        assert sum(map(len, case.docs)) < 100_000, name


@pytest.mark.parametrize("fold", [False, True])
def test_oracle_is_not_trivial(fold):
    for name, case in ub.cases().items():
        mo, ti, po = ub.expected_csr(name, fold)
        per_doc = np.diff(mo.astype(np.int64))
        assert ti.size >= 40 and np.count_nonzero(per_doc) >= 20, name
        assert len(set(ti.tolist())) >= 8, name
        rows = ub.expected_rows(name, fold)
        bits = np.unpackbits(rows.view(np.uint8), axis=1, bitorder="little")[:, :len(ub.EXPRESSIONS)]
        assert 0.02 <= bits.mean() <= 0.9, name
        assert bits.any(axis=0).sum() >= 10, name
    # folding finds more: the documents spell keywords in mixed case
    assert ub.expected_csr("pairs", True)[1].size > ub.expected_csr("pairs", False)[1].size
    # the oracle agrees with brute force on the batch with the most borders
    docs = ub.cases()["long_doc"].docs
    want = brute_force(ub.TERMS, docs, POS_START, fold)
    for a, b in zip(ub.expected_csr("long_doc", fold), want):
        assert np.array_equal(a, b)


def test_pairs_cover_every_length_and_class_pair():
    docs = ub.cases()["pairs"].docs
    assert {len(d) for d in docs} == set(ub.LENGTHS)
    every = {(a, b) for a in range(len(ub.CLASSES)) for b in range(len(ub.CLASSES))}
    assert ub.pair_coverage(docs, 1) == every and ub.pair_coverage(docs, ub.WAVES) == every
    assert len(docs) % ub.WAVES == 0 and len(docs) // ub.WAVES >= 10
    # an empty document as the next unit, and a next unit of fewer than 64 x 4 bytes, behind every class
    assert {a for a, b in ub.pair_coverage(docs, ub.WAVES) if b == 0} == set(range(len(ub.CLASSES)))
    assert all(max(c) < 256 for c in ub.CLASSES[:4])
    # the tiny documents hold keywords at offsets 0 .. 2 (the short terms' start rule)
    mo, ti, po = ub.expected_csr("pairs", False)
    tiny = [d for d, doc in enumerate(docs) if 1 <= len(doc) <= 5 and mo[d + 1] > mo[d]]
    assert len(tiny) >= 10


@pytest.mark.parametrize("lead_len", ub.LEADS)
def test_empty_run(lead_len):
    case = ub.cases()["empty_run_lead%d" % lead_len]
    assert case.docs[:20] == [b""] * 20 and len(case.lead) == lead_len
    first = case.docs[20]
    buf, off, at = ub.placed(case.name)
    assert int(off[0]) == lead_len and int(off[20]) == lead_len and int(off[21]) == lead_len + len(first)
    # keywords in the first bytes of the document at blob offset doc_off[0] < 4
    mo, ti, po = ub.expected_csr(case.name, False)
    assert sorted(po[int(mo[20]):int(mo[21])].tolist())[:3] == [0, 0, 2]               # "7" and "7.7" at offset 0, "7" at 2
    if lead_len:
        # read as one text the lead bytes complete "q7" across doc_off[0] (and hold "q", "zx", "zxq" in front of it)
        whole = bytes(buf[:int(off[-1])])
        assert whole[lead_len - 1:lead_len + 1] == b"q7"
        n_whole = brute_force(ub.TERMS, [whole], POS_START, False)[1].size
        assert n_whole > ti.size


def test_blob_end():
    case = ub.cases()["blob_end"]
    buf, off, at = ub.placed(case.name)
    end = int(off[-1])
    text = bytes(buf[:end])
    assert text.endswith(b"nation") and len(case.tail) < 64
    behind = bytes(buf[end:end + 64])
    assert (text[-6:] + behind).startswith(ub.pl.E33)                                   # "nationwide slack behind the blobs"
    mo, ti, po = ub.expected_csr(case.name, False)
    names = sorted(set(ub.TERMS))
    last = {names[t] for t in ti[int(mo[-2]):].tolist()}
    assert {b"nation", b"tion"} <= last and not {ub.pl.E10, ub.pl.E33, b"nations"} & last
    n_whole = brute_force(ub.TERMS, [text + behind], POS_START, False)[1].size
    assert n_whole >= ti.size + 2                                                       # E10 and E33 lie across the blob's end


def test_long_doc_borders_and_density():
    case = ub.cases()["long_doc"]
    d = next(i for i, doc in enumerate(case.docs) if len(doc) == ub.LONG_DOC)
    assert 0 < d < len(case.docs) - 1 and sum(len(x) == ub.LONG_DOC for x in case.docs) == 1
    doc = case.docs[d]
    planted = ub.long_doc_planted()
    borders = {b for b, _, _ in planted}
    for unit_max in ub.UNIT_SIZES:
        assert set(ub.unit_borders(ub.LONG_DOC, unit_max)) <= borders
    assert len(ub.unit_borders(ub.LONG_DOC, 8192)) == 4 and len(ub.unit_borders(ub.LONG_DOC, 512)) == 78
    mo, ti, po = ub.expected_csr(case.name, False)
    names = sorted(set(ub.TERMS))
    found = set(zip(po[int(mo[d]):int(mo[d + 1])].tolist(), (names[t] for t in ti[int(mo[d]):int(mo[d + 1])].tolist())))
    for b, start, t in planted:
        assert start < b < start + len(t) and doc[start:start + len(t)] == t           # across the border, not overwritten
        assert (start, t) in found, (b, start, t)
    assert {len(t) for _, _, t in planted} >= {2, 3, 4, 10, 24, 26, 33, 300}
    # both kinds of scan learn 512-byte units from this batch: with positions (matches) and presence-only (pool entries)
    blob, off = pack_strings(case.docs)
    once, matches = Model(ub.TERMS).entries(blob, off, 8192, False)
    assert matches == ti.size
    for total in (matches, once):
        assert learned_unit(KERNEL, FIFO_CAP, total, 0, int(off[-1])) == 512


def test_second_walk_outgrows_the_fifo():
    case = ub.cases()["second_walk"]
    blob, off = pack_strings(case.docs)
    per_doc, _ = Model(ub.TERMS).per_doc(blob, off, 8192, False)
    big = [i for i, n in enumerate(per_doc) if n > FIFO_CAP]
    assert len(big) == 2 and all(len(case.docs[i]) <= 8192 for i in big)               # one unit each
    assert big[0] >= ub.WAVES and len(case.docs) - big[1] > 8                           # a next unit of some wave; ordinary units follow
    assert all(n < FIFO_CAP for i, n in enumerate(per_doc) if i not in big)
    mo = ub.expected_csr(case.name, False)[0]
    assert all(int(mo[i + 1] - mo[i]) > FIFO_CAP for i in big)
