"""The model of tests/presence_once.py -- what a presence-only scan writes to the match pool -- against cases counted by hand,
and the documents of tests/test_gpu_presence_once.py against what they are meant to exercise.  No GPU."""
import numpy as np

import presence_once as po
from helpers import docs, scan_plan


def entries(model, text, unit_max=8192):
    blob, off = docs([text])
    return model.entries(blob, off, unit_max)


def test_a_term_that_repeats_is_one_entry():
    m = po.Model([b"ab", b"wxyz"])
    assert entries(m, po.repeats(b"ab", 200)) == (1, 200)
    assert entries(m, po.repeats(b"ab", 1)) == (1, 1)
    # the first occurrence ends at offset 1: it is written as a match, the record once more for the 199 behind it
    assert entries(m, b"ab" + po.repeats(b"ab", 199)) == (2, 200)
    assert entries(m, b"ab") == (1, 1) and entries(m, b"") == (0, 0)
    # long terms are written every time
    assert entries(m, po.fill(8) + b"wxyz" * 50) == (50, 50)


def test_sets_of_the_test_dictionary():
    m = po.Model(po.TERMS)
    c = po.single_unit_cases(256)
    assert entries(m, c["cab_x65"]) == (3, 3 * 65)                       # {cab, ab, b} once
    assert entries(m, c["ab_x2"]) == (2, 4) and entries(m, c["de_x200"]) == (1, 200)
    assert entries(m, c["ab_then_cab"]) == (2 + 3, 5)                    # ab, b at offset 1 as matches; {cab, ab, b} later
    assert entries(m, c["cab_then_ab"]) == (3 + 2, 5)                    # cab, ab, b at offset 2 as matches; {ab, b} later
    assert entries(m, c["ab_at_start_then_ab"]) == (2 + 2, 6)
    assert entries(m, c["three_sets"]) == (3 + 3 + 2 + 1, 3 + 3 + 2 + 1 + 3 + 3)
    assert entries(m, c["b_alone"]) == (1, 1) and entries(m, c["ab_alone"]) == (2, 2)
    assert entries(m, c["no_short_term"]) == (4, 4) and entries(m, c["empty"]) == (0, 0)    # hgfe (filler + e), efgh, aceg, aceghf
    got, matches = entries(m, c["second_walk"])
    assert matches > 256 + 64 and matches - got > 256                    # more long matches than the fifo holds, and repeats


def test_units_count_on_their_own():
    m = po.Model(po.TERMS)
    assert po.unit_bytes(po.LONG_DOC, 8192) == 6667 and po.unit_bytes(po.LONG_DOC, 512) == 500
    for where in ("first", "last"):
        assert entries(m, po.long_doc(where), 8192) == (3, 6) and entries(m, po.long_doc(where), 512) == (3, 6)
    big, matches = entries(m, po.long_doc("all"), 8192)
    small, _ = entries(m, po.long_doc("all"), 512)
    # three units hold each of the four sets once (9 entries a unit); forty units of 500 bytes hold two spots each
    assert big == 3 * 9 and small > big and small <= matches


def test_documents_reach_the_paths_they_name():
    kernel, plan = scan_plan(po.TERMS)
    assert kernel == "scan5"
    fifo = plan["fifo_cap"]
    c = po.single_unit_cases(fifo)
    n = max(200, fifo // 2 + 72)
    assert c["ab_x%d" % n].count(b"ab") == n > fifo // 2                 # parked jobs of one pass outgrow half the fifo
    # ONE pass: the early drain in park_short needs all those jobs parked in one pass of the candidate list, i.e. the unit's
    # flagged positions within cand_cap.  gft_debug_scan_plan does not hand cand_cap out; scan5_plan gives this dictionary (a
    # dozen byte classes, a filter of a few KB) the list's ceiling of 2 048 entries, and the documents are shorter than that
    assert all(len(c["%s_x%d" % (t, n)]) < 2048 for t in ("ab", "cab", "de"))
    assert c["second_walk"].count(b"abcd") > fifo
    m = po.Model(po.TERMS)
    blob, off = docs([po.DENSE])
    got, _ = m.entries(blob, off, 8192)
    from helpers import learned_unit
    assert learned_unit("scan5", fifo, got, 0, len(po.DENSE)) == 512   # what the handle learns from the dense call
    sets = {frozenset(s) for s in ([b"cab", b"ab", b"b"], [b"xab", b"ab", b"b"], [b"ab", b"b"])}
    assert len(sets) == 3 and np.all([len(t) <= 3 for t in po.SHORT_TERMS])
