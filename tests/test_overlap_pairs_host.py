"""The overlap checks of the resident-batch calls, pair by pair, through the host walks (gft_debug_*), which ask the same per-call
functions as the device entry points: every output against every input and every other output of its call, once sharing one
element (refused, nothing written) and once adjacent (taken, the disjoint call's answer).  Cases, pair lists and what to expect:
tests/overlap_pairs.py.  No device needed."""
import pytest

import overlap_pairs as P


def test_the_calls_and_their_pairs():
    """twelve calls; the variants of a call are two for every (output, other range) pair, none left out"""
    assert [c.name for c in P.CALLS] == ["excerpt", "excerpt_snap", "mark", "replace", "select", "route", "context", "words", "term_stats", "columns",
                                         "hit_spans", "to_lower"]
    for c in P.CALLS:
        assert len(list(P.variants(c))) == 2 * P.n_pairs(c)
        assert all(r.nbytes >= 2 for r in c.ranges)
    assert {c.name: P.n_pairs(c) for c in P.CALLS} == {"excerpt": 77, "excerpt_snap": 77, "mark": 32, "replace": 66, "select": 18, "route": 45,
                                                       "context": 45, "words": 36, "term_stats": 12, "columns": 1, "hit_spans": 28, "to_lower": 6}


@pytest.mark.parametrize("call", P.CALLS, ids=[c.name for c in P.CALLS])
def test_every_pair(call):
    base = P.host_base(call)
    for label, at, refused in P.variants(call):
        rc, before, after = P.run_host(call, at)
        P.check(call, label, at, refused, rc, before, after, base)
