"""The overlap checks of the resident-batch calls, pair by pair, through the device entry points: the cases and pairs of
tests/overlap_pairs.py (what tests/test_overlap_pairs_host.py puts the host walks through) on tensors carved from one device arena,
one engine for the file.  Every output against every input and every other output of its call, once sharing one element (refused,
nothing written) and once adjacent (taken); after every refusal one valid call on the same handle.  Every answer is compared with the
host walk's answer for the disjoint call.

What a device call takes in host memory (the route's masks and bucket arrays) lives in a host arena of the same layout: a pair
across the two cannot be made to meet and is the host file's alone.  gft_hit_spans_device scans a text before it checks -- other
inputs than the walk behind it has -- and stays with the host file too.  The shapes are the smallest there are: the code under test
is argument logic and one read-back; the run passes' tile and trip borders are in the span calls' own files."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (before libgft.so is loaded: one HIP runtime)

import overlap_pairs as P
from gofindthem_amd import _lib
from gofindthem_amd.engine import Engine

pytestmark = pytest.mark.gpu

L = _lib.load()
CALLS = [c for c in P.CALLS if c.device]


@pytest.fixture(scope="module")
def eng():
    e = Engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def arena():
    return torch.empty(max(P.arena_bytes(c) for c in CALLS), dtype=torch.uint8, device="cuda")


def run_device(call, eng, arena, at):
    """the device entry point on the arena: (rc, bytes before, bytes after), the host arena's ranges laid over the device's"""
    size = P.arena_bytes(call)
    before = P.prepare(call, at, size)
    arena[:size].copy_(torch.from_numpy(before))
    host = before.copy()
    ptr = {r.name: (host.ctypes.data if r.space == "host" else arena.data_ptr()) + at[r.name] for r in call.ranges}
    rc = call.invoke(functools.partial(getattr(L, call.device), eng._h), ptr)
    torch.cuda.synchronize()
    after = arena[:size].cpu().numpy()
    hosted = np.zeros(size, bool)
    for r in call.ranges:
        if r.space == "host":
            hosted[at[r.name]:at[r.name] + r.nbytes] = True
    assert np.array_equal(after[hosted], before[hosted]) and np.array_equal(host[~hosted], before[~hosted]), "%s: a write in the wrong memory" % call.name
    after[hosted] = host[hosted]
    return rc, before, after


def test_the_calls():
    assert [c.name for c in CALLS] == ["excerpt", "excerpt_snap", "mark", "replace", "select", "route", "context", "words", "term_stats", "columns",
                                       "to_lower"]


@pytest.mark.parametrize("call", CALLS, ids=[c.name for c in CALLS])
def test_every_pair(eng, arena, call):
    base = P.host_base(call)
    home = P.homes(call)
    rc, before, after = run_device(call, eng, arena, home)
    P.check(call, call.name + ": disjoint", home, False, rc, before, after, base)
    spaces = {r.name: r.space for r in call.ranges}
    n = 0
    for label, at, refused in P.variants(call, spaces):
        rc, before, after = run_device(call, eng, arena, at)
        P.check(call, label, at, refused, rc, before, after, base)
        if refused:
            rc, before, after = run_device(call, eng, arena, home)
            P.check(call, label + ", then a valid call", home, False, rc, before, after, base)
        n += 1
    across = sum(1 for o in call.ranges if o.role == "out" for x in call.ranges if x is not o and x.space != o.space)
    assert n == 2 * (P.n_pairs(call) - across)
