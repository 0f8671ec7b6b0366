"""scan_modes.py on the CPU: the two rune references agree on every string of the sweep, the cases hold what they claim
(assert_not_vacuous lists, for every wrong reading of the two contracts, the cases that would catch it), bytes.find finds what the
oracle finds, and the inputs of the older rune test read the same through both references."""
import itertools

import numpy as np

import scan_modes as sm
from oracle import runes_ref
from oracle.pyoracle import POS_END, POS_START


def _sweep(length):
    bad = []
    for s in itertools.product(sm.ALPHABET, repeat=length):
        b = bytes(s)
        if sm.rune_table(b).tolist() != runes_ref.rune_index_table(b):
            bad.append(b.hex())
    return bad


def test_strict_decoder_walk_equals_the_table_walk_up_to_three_bytes():
    """every string of 0 to 3 bytes over the 24-byte alphabet (14 425 strings): Python's strict decoder against the acceptance
    table of oracle/runes_ref.py"""
    for n in range(4):
        assert not _sweep(n), n


def test_strict_decoder_walk_equals_the_table_walk_at_four_bytes():
    """the 331 776 strings of four bytes: every four-byte form, whole, broken at each byte, and followed or preceded by any byte.
    By first byte, so that a failure names it"""
    for first in sm.ALPHABET:
        bad = []
        for s in itertools.product(sm.ALPHABET, repeat=3):
            b = bytes((first,) + s)
            if sm.rune_table(b).tolist() != runes_ref.rune_index_table(b):
                bad.append(b.hex())
        assert not bad, (hex(first), bad[:5])


def test_reference_on_known_strings():
    """the reference against answers written by hand (Go: []rune of each)"""
    t = sm.rune_table
    assert t(b"").tolist() == [0]
    assert t("aé€\U0001d11eb".encode()).tolist() == [0, 1, 2, 2, 3, 3, 3, 4, 4, 4, 4, 5]     # inside a rune: that rune has started
    assert t(b"\xe2\x82").tolist() == [0, 1, 2] and t(b"\xed\xa0\x80").tolist() == [0, 1, 2, 3]
    assert t(b"\xf0\x9d\x84\x9e\x80").tolist() == [0, 1, 1, 1, 1, 2] and t(b"\xc0\x80").tolist() == [0, 1, 2]
    assert t(b"\xf4\x90\x80\x80").tolist() == [0, 1, 2, 3, 4] and t(b"\xf4\x8f\xbf\xbf").tolist() == [0, 1, 1, 1, 1]
    # ... and the wrong readings are wrong where they should be
    assert sm.table_replace(b"\xe2\x82x").tolist() == [0, 1, 1, 2]                           # one replacement character for two bytes
    assert sm.table_blocks(b"a" * 63 + "é".encode()).tolist()[-2:] == [64, 65]               # the rune's second byte starts block 1
    assert [x.tolist() for x in sm.tables_unbounded(b"\xc3", [b"\xa9a"], b"")] == [[0, 0, 1]]


def test_cases_are_not_vacuous():
    caught = sm.assert_not_vacuous()
    for what, names in caught.items():
        print("%-40s %4d: %s" % (what, len(names), "; ".join(names[:4])))
    assert len(caught) == 7 + len(sm.GRIDS)


def test_bytes_find_finds_what_the_oracle_finds():
    """the full match lists of the small fixed cases by bytes.find: per document the oracle's multiset, in both position modes"""
    for c in sm.small_rune_cases() + [sm.unique_fixed()]:
        for mode in (POS_START, POS_END):
            want, got = sm.full_csr(c, mode), sm.brute_csr(c, mode)
            assert np.array_equal(want[0], got[0]), (c.name, mode)
            assert sm.per_document_multisets(want) == sm.per_document_multisets(got), (c.name, mode)
            # (long_terms.brute_force also claims the canonical order)
            assert np.array_equal(want[1], got[1]) and np.array_equal(want[2], got[2]), (c.name, mode)


def test_the_older_rune_test_reads_the_same_through_both_references():
    """the inputs of test_gpu_parity.test_rune_offsets_are_the_anknown_engine_positions"""
    from gofindthem_amd.workload import Workload
    raw = sm.parity_rune_texts()
    w = Workload(300, alphabet="mixed")
    text, off = w.docs_host(0, 40)
    raw += [bytes(text[int(off[d]):int(off[d + 1])]) for d in range(40)]
    assert any(max(r, default=0) >= 0x80 for r in raw[6:])
    for r in raw:
        assert sm.rune_table(r).tolist() == runes_ref.rune_index_table(r), r[:40]
    # the placement module's rune leg
    import placement as pl
    for doc in pl.batch("short_mixed").docs:
        assert sm.rune_table(doc).tolist() == runes_ref.rune_index_table(doc)
