"""placement.py is what it claims (no GPU): the surroundings hold what a scan must not take for text, `place` puts the documents
where doc_off says, the oracle agrees with the brute force on the bare documents, and no expectation knows of a placement."""
import numpy as np
import pytest

import placement as pl
from helpers import assert_csr_equal
from long_terms import brute_force
from oracle.pyoracle import Oracle, pack_strings


def test_the_surroundings_are_hostile():
    pl.assert_not_vacuous()


@pytest.mark.parametrize("name", ["long", "long_mixed"])
@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("pos_mode", pl.POS_MODES)
def test_oracle_scan_is_the_brute_force_on_the_bare_documents(name, fold, pos_mode):
    b = pl.batch(name)
    blob, off = pack_strings(b.docs)
    assert off[0] == 0
    got = Oracle(b.terms, pos_mode).scan(blob, off, fold=fold)
    assert_csr_equal(got, pl.expected_csr(name, pos_mode, fold))
    assert got[1].size > 2000
    again = brute_force(b.terms, b.docs, pos_mode, fold)
    assert_csr_equal(again, pl.expected_csr(name, pos_mode, fold))


@pytest.mark.parametrize("name", pl.BATCHES)
def test_place_puts_the_documents_where_doc_off_says(name):
    b = pl.batch(name)
    for kind in pl.KINDS:
        for at, lead_len in pl.PLACEMENTS:
            buf, off, start = pl.placed(name, kind, at, lead_len)
            lead, tail = pl.surroundings(kind, lead_len, b)
            assert start == at and int(off[0]) == lead_len == len(lead) and off.dtype == np.uint64 and len(off) == len(b.docs) + 1
            raw = buf.tobytes()
            assert raw[:at] == bytes([pl.FILL]) * at and raw[at:at + lead_len] == lead
            text = raw[at:]
            for d, doc in enumerate(b.docs):
                assert text[int(off[d]):int(off[d + 1])] == doc
            end = int(off[-1])
            assert text[end:end + len(tail)] == tail
            assert len(text) >= end + pl.SLACK + 16 and set(text[end + max(len(tail), pl.SLACK):]) == {pl.FILL}


def test_expectations_do_not_depend_on_the_placement():
    """trivially so -- they are computed from the bare documents --, and asserted so that it stays so: the same objects before and
    behind every placement, and equal to what a fresh computation gives"""
    for name in ("short", "long"):
        b = pl.batch(name)
        before = {(m, f): pl.expected_csr(name, m, f) for m in pl.POS_MODES for f in (False, True)}
        rows = {(w, f): pl.expected_rows(name, w, f) for w in (pl.PRESENCE, pl.POSITIONS) for f in (False, True)}
        for kind in pl.KINDS:
            for at, lead_len in pl.PLACEMENTS:
                pl.placed(name, kind, at, lead_len)
                for k, v in before.items():
                    assert pl.expected_csr(name, *k) is v and not v[1].flags.writeable
                for k, v in rows.items():
                    assert pl.expected_rows(name, *k) is v and not v.flags.writeable
        assert_csr_equal(brute_force(b.terms, b.docs, pl.POS_MODES[0], True), before[(pl.POS_MODES[0], True)])
        assert rows[(pl.PRESENCE, True)].shape == (len(b.docs), (len(pl.expressions(pl.PRESENCE)) + 31) // 32)
        assert np.array_equal(rows[(pl.POSITIONS, True)][:, :2], rows[(pl.PRESENCE, True)][:, :2])       # (the first 64 expressions are shared)
        assert 0 < int(np.unpackbits(rows[(pl.POSITIONS, False)].view(np.uint8)).sum()) < rows[(pl.POSITIONS, False)].size * 32


def test_fold_safe_is_the_rule_of_gft_last_nonascii():
    assert pl.fold_safe(b"plain") and pl.fold_safe("café straße ×".encode()) and pl.fold_safe(b"\xc2\x89")
    for bad in ("École".encode(), "€".encode(), b"\xa9x", b"x\xc3", b"x\xc2", b"\xc3\xc3\xa9", b"\xff"):
        assert not pl.fold_safe(bad), bad
