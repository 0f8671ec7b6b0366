"""The two users of the bit-row walk (csrc/gft_bitrows_dev.hpp) on one bitmap: gft_compact_device, a row a document, and
gft_debug_tag_entries_device, a row a leaf with one leaf per record and every field valid.  Both must give the same lists, bit for
bit, and both the numpy restatement below."""
import numpy as np
import pytest
import torch  # noqa: F401  (before libgft.so is loaded: one HIP runtime)

import records as R
from test_gpu_sparse import CANARY, compact, engine_with
from test_gpu_tags import GUARD_DEV, dev, host, make_group

pytestmark = pytest.mark.gpu

N_ROWS = 130          # more than two groups at 64 rows a wave and trip, a partial last group at every segment width
N_FIELDS = 8


def make_bitmap(n_exprs, rng):
    """rows of about 10 % set bits, row 0 empty and row 1 full; every bit at and above n_exprs in the last word set"""
    words = (n_exprs + 31) // 32
    bits = rng.random((N_ROWS, words * 32)) < 0.1
    bits[0], bits[1] = False, True
    assert n_exprs % 32, "the shapes of this file leave room for garbage in the last word"
    bits[:, n_exprs:] = True
    return np.packbits(bits, axis=1, bitorder="little").view(np.uint32).reshape(N_ROWS, words)


def numpy_lists(bm, n_exprs, field):
    bits = np.unpackbits(bm.view(np.uint8), bitorder="little").reshape(N_ROWS, -1)[:, :n_exprs]
    rows, cols = np.nonzero(bits)
    row_off = np.concatenate([[0], np.cumsum(bits.sum(axis=1))]).astype(np.uint64)
    return row_off, cols.astype(np.uint32), field[rows]


@pytest.mark.parametrize("n_exprs", [1, 33, 95, 2043, 2085, 4123])
def test_documents_and_tag_entries_walk_one_bitmap_alike(n_exprs):
    """words a row: 1, 2, 3 (an idle lane in a segment of four), 64, 66 (carry, partial second step), 129"""
    rng = np.random.default_rng(n_exprs)
    bm = make_bitmap(n_exprs, rng)
    field = rng.integers(0, N_FIELDS, N_ROWS).astype(np.uint32)
    rec_off = np.arange(N_ROWS + 1, dtype=np.uint64)
    want_off, want_expr, want_field = numpy_lists(bm, n_exprs, field)
    total = int(want_off[-1])
    assert want_off[1] == 0 and want_off[2] == n_exprs and total > n_exprs

    V = R.vocabulary()
    e = engine_with(n_exprs)
    g = make_group(['"%s"' % V[i % len(V)] for i in range(n_exprs)], ["tag%d" % (i % 7) for i in range(n_exprs)], R.make_schema(N_FIELDS))
    d_bm, d_field, d_off = dev(bm.view(np.int32), np.int32), dev(field, np.int32), dev(rec_off, np.int64)
    for cap in (total, total // 2):
        what = "n_exprs=%d cap=%d of %d" % (n_exprs, cap, total)
        row_off, expr_idx, _, t = compact(e, bm, N_ROWS, cap, False, slack=total + 64)
        t_off, ent_field, ent_expr, _, t_total = host(g.debug_tag_entries_device(d_bm, n_exprs, d_field, d_off, cap=cap, want_tag=False))
        t_off, ent_field, ent_expr = t_off.astype(np.uint64), ent_field.view(np.uint32), ent_expr.view(np.uint32)
        assert t == total and t_total == total, what
        assert np.array_equal(row_off, t_off) and np.array_equal(row_off, want_off), what
        assert np.array_equal(ent_expr[:cap], expr_idx[:cap]) and np.array_equal(expr_idx[:cap], want_expr[:cap]), what
        assert np.array_equal(ent_field[:cap], want_field[:cap]), what
        assert (expr_idx[cap:] == CANARY).all(), what
        assert ent_expr.size == cap + g.GUARD and (ent_expr[cap:] == GUARD_DEV).all() and (ent_field[cap:] == GUARD_DEV).all(), what
    g.close()
    e.close()
