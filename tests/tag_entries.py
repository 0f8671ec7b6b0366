"""Helpers of the tag entry tests (test_tags_host.py, test_gpu_tags.py): the restatement of the contract of include/gft.h's tag
entries -- from a leaf hit bitmap (records.Expectation.hit_bitmap: the CPU oracle's ProcessText per leaf) and
oracle/group_ref.py's is_valid_field_path --, seeded batches that are not vacuous, and the comparison of a result with it.  No
tests in here."""
import numpy as np

import records as R
from oracle import group_ref

GUARD_HOST = 0xA5A5A5A5          # what gofindthem_amd.group fills the host arrays with; the device arrays hold -1
EVERYTHING = " ".join(R.vocabulary())            # a leaf that makes every expression of records.make_expressions true


def valid_fields(schema, include, exclude):
    return [group_ref.is_valid_field_path(p, include, exclude) for p in schema]


def expected(hits, E, field, rec_off, valid):
    """-> (row_off u64[n + 1], ent_field u32[], ent_expr u32[], stats): leaves in record order, expressions ascending inside a
    leaf, one entry per set bit e < E of a leaf whose field is valid.  stats: leaves that contribute nothing, hits (bits < E) in
    invalid fields"""
    hits = np.ascontiguousarray(hits, dtype=np.uint32).reshape(len(field), (E + 31) // 32)
    bits = np.unpackbits(hits.view(np.uint8), axis=1, bitorder="little")[:, :E] if len(field) and E else np.zeros((len(field), E), np.uint8)
    row_off, ef, ee = [0], [], []
    silent = masked = 0
    for r in range(len(rec_off) - 1):
        for l in range(int(rec_off[r]), int(rec_off[r + 1])):
            f = int(field[l])
            on = np.flatnonzero(bits[l])
            if not valid[f]:
                masked += len(on)
                on = on[:0]
            silent += len(on) == 0
            ef += [f] * len(on)
            ee += [int(e) for e in on]
        row_off.append(len(ee))
    return (np.asarray(row_off, dtype=np.uint64), np.asarray(ef, dtype=np.uint32), np.asarray(ee, dtype=np.uint32),
            {"total": len(ee), "silent": silent, "masked": masked})


def assert_not_vacuous(stats, masked=True):
    assert stats["total"] > 0
    assert stats["silent"] > 0                       # at least one leaf contributes nothing
    if masked:
        assert stats["masked"] > 0                   # an excluded field carried a hit that must not appear


def assert_entries(got, want, expr_tag, cap=None, guard=GUARD_HOST):
    """got: (row_off, ent_field, ent_expr, ent_tag or None, total) with the arrays a guard longer than cap; want: expected()'s"""
    row_off, ef, ee, et, total = got
    w_off, w_f, w_e, stats = want
    assert total == stats["total"]
    assert np.array_equal(np.asarray(row_off).astype(np.uint64), w_off)       # complete whatever the cap
    cap = total if cap is None else cap
    n = min(cap, total)
    cols = [(ef, w_f), (ee, w_e)] + ([(et, np.asarray(expr_tag, dtype=np.uint32)[w_e])] if et is not None else [])
    for col, w in cols:
        col = np.asarray(col).astype(np.uint32)
        assert len(col) > cap                                                  # (there are guard words to look at)
        assert np.array_equal(col[:n], w[:n])
        assert (col[n:] == np.uint32(guard)).all()                             # nothing stored at or past the cap, nor behind it


def planted_records(N, schema, rng, valid, max_leaves=4):
    """records.make_records plus what makes a batch not vacuous whatever the seed: a leaf that matches everything in every
    invalid field and in one valid field, an empty-string leaf, an empty record first, in the middle and last"""
    recs = R.make_records(N, schema, rng, max_leaves=max_leaves)
    bad = [p for p, ok in zip(schema, valid) if not ok]
    good = [p for p, ok in zip(schema, valid) if ok]
    extra = [[(p, EVERYTHING)] for p in bad]
    if good:
        extra.append([(good[0], ""), (good[-1], EVERYTHING), (good[0], "")])
    for k, rec in enumerate(extra):
        recs.insert(min(len(recs), 1 + 3 * k), rec)
    return [[]] + recs[:len(recs) // 2] + [[]] + recs[len(recs) // 2:] + [[]]


def tag_maps(exp, records, hits=None):
    """the oracle's tag map of every record ({tag: {field: sorted expressions}}): records.Expectation.rules_of's"""
    _, maps = exp.rules_of(records, hits)
    return [{t: {f: sorted(v) for f, v in fs.items()} for t, fs in m.items()} for m in maps]
