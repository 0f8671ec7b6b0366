"""tests/unit_chain.py builds what it claims (no GPU): the unit counts around the 16 waves of a workgroup, documents that are two
and three units with keywords across the borders, lead bytes and slack that would complete a keyword, two dictionaries on both
sides of 32 byte classes, a batch beyond the smallest match pool -- and expectations that are not vacuous."""
import numpy as np
import pytest

import placement as pl
import unit_chain as uc
from oracle.pyoracle import POS_START, Oracle, pack_strings
from presence_once import unit_bytes

UNIT_MAX = 8192                                          # a fresh engine's


def test_dictionaries_on_both_sides_of_32_classes():
    assert uc.classes(uc.TERMS_SMALL) <= 32 < uc.classes(uc.TERMS_LARGE)
    assert set(uc.TERMS_SMALL) <= set(uc.TERMS_LARGE)
    for terms in uc.DICTIONARIES.values():
        assert len(set(terms)) == len(terms)
        have = pl.length_classes(terms)
        assert all(have[c] for c in ("1-3", "4", "5-24", "25-28", "29-40", "long")), have


def test_unit_counts():
    c = uc.cases()
    want = {"one": 1, "few": 5, **{"n%d" % n: n for n in uc.COUNTS}}
    for name, n in want.items():
        docs = c[name].docs
        assert len(docs) == n and all(0 < len(d) <= 512 for d in docs), name      # one unit each, at every unit size
    assert c["few"].docs and len(c["few"].docs) < uc.WAVES
    assert {n % uc.WAVES for n in uc.COUNTS} == {15, 0, 1} and max(uc.COUNTS) > 3 * uc.WAVES
    assert c["last_empty"].docs[-1] == b"" and c["last_empty"].docs[-2] and c["first_empty"].docs[0] == b"" and c["first_empty"].docs[1]


@pytest.mark.parametrize("n", uc.LONG_DOCS)
def test_long_documents_are_cut_inside_keywords(n):
    docs = uc.cases()["doc%d" % n].docs
    (d,) = [x for x in docs if len(x) > 512]
    assert len(d) == n and docs.index(d) not in (0, len(docs) - 1)
    per = unit_bytes(n, UNIT_MAX)
    borders = list(range(per, n, per))
    assert len(borders) == (n - 1) // UNIT_MAX and borders      # two units and three: the later ones begin at lo > 0
    m_off, term, pos = uc.oracle("small").scan(*pack_strings([d]), fold=False)
    terms = sorted(set(uc.TERMS_SMALL))
    for b in borders:
        assert any(p < b < p + len(terms[t]) for t, p in zip(term.tolist(), pos.tolist())), b
    assert uc.LONG_TERM in d


def _matches(o, text, fold=False):
    return o.scan(*pack_strings([text]), fold=fold)[1].size


def test_lead_bytes_and_slack_would_complete_a_keyword():
    o = Oracle(uc.TERMS_SMALL, POS_START)
    for k in uc.LEADS:
        c = uc.cases()["lead%d" % k]
        buf, off, start = uc.placed(c.name)
        assert start == 0 and int(off[0]) == k and bytes(buf[:k]) == c.lead
        first = c.docs[0]
        assert first[:3] == b"7.7"
        if k:
            assert _matches(o, c.lead + first) > _matches(o, first), k
    c = uc.cases()["blob_end"]
    buf, off, start = uc.placed("blob_end")
    text = b"".join(c.docs)
    assert int(off[-1]) == len(text) and c.docs[-1].endswith(b"nation")
    assert _matches(o, c.docs[-1] + c.tail[:27]) > _matches(o, c.docs[-1])
    assert len(buf) >= int(off[-1]) + 64


def test_expectations_are_not_vacuous():
    n_terms = len(sorted(set(uc.TERMS_SMALL)))
    for name, c in uc.cases().items():
        for which in uc.DICTIONARIES:
            raw, fold = uc.expected_csr(name, which, False), uc.expected_csr(name, which, True)
            assert raw[1].size and fold[1].size >= raw[1].size, (name, which)
            rows = uc.expected_rows(name, which, True)
            assert rows.shape[0] == len(c.docs) and rows.any(), (name, which)
    # the large dictionary's own keywords never occur in the ASCII documents: the same matches under other term ids
    a, b = uc.expected_csr("n49", "small", True), uc.expected_csr("n49", "large", True)
    assert np.array_equal(a[0], b[0]) and n_terms == len(uc.expressions()) - 7
    assert any(fold[1].size > raw[1].size for raw, fold in ((uc.expected_csr(n, "small", False), uc.expected_csr(n, "small", True)) for n in uc.cases()))


@pytest.mark.parametrize("fold", [False, True], ids=["raw", "fold"])
def test_pool_case_outgrows_the_smallest_pool(fold):
    docs, want, entries = uc.pool_case(fold)
    assert len(docs) == uc.POOL_DOCS == want.shape[0] and entries > uc.POOL_MIN + uc.POOL_MIN // 8
    assert sum(map(len, docs)) // 16 < uc.POOL_MIN       # (the pool is not sized by the text either)
    assert want.any(axis=1).all() and not want.all()
