"""Tag entries, host half: gft_debug_tag_entries (csrc/tag_entries.cpp -- the contract of the tag kernels in plain loops, and the
second route of gft_group_tag_records) against the restatement of tests/tag_entries.py over leaf bitmaps taken from the CPU
oracle, and tags_from_entries against oracle/group_ref.py's tag_object.  Nothing here needs a GPU.

Every generated batch asserts that it is not vacuous (tag_entries.assert_not_vacuous): entries exist, some leaf contributes
nothing, some excluded field carried a hit that must not appear.  The cases that are degenerate by construction (no records, no
leaves, every leaf invalid, a schema of one field, which cannot have an excluded field beside a valid one) say what they are."""
import os

import numpy as np
import pytest

import records as R
import tag_entries as TE
from gofindthem_amd import _lib, group
from gofindthem_amd.finder import Finder, PyRegexpEngine
from oracle import group_ref


def tag_ids(tags):
    ids = {}
    return [ids.setdefault(t, len(ids)) for t in tags]          # numbered by first appearance (Finder::tags)


def make_group(exprs, tags, schema, include=None, exclude=None, rules=None, rgx=None):
    f = Finder(None, rgx, False, allow_no_device=True)
    for e, t in zip(exprs, tags):
        f.AddExpressionWithTag(e, t)
    g = group.NewFinderWithRules(f, rules or {})
    g.SetSchema(schema, include, exclude)
    return g


def lists_for(schema):
    """an exclude list that takes out the fields at indices 31 and 32 where the schema has them (the word border of the mask),
    else its last field; a schema of one field keeps it"""
    F = len(schema)
    if F == 1:
        return None, None
    return None, [schema[i] for i in (31, 32) if i < F] if F > 31 else [schema[-1]]


class Case:
    """one (E, F) configuration with its oracle hits, computed once and left unchanged"""

    def __init__(self, E, F, seed=0, N=40, include=None, exclude=None, lists=True):
        rng = np.random.default_rng([seed, E, F])
        self.schema = R.make_schema(F)
        if lists:
            include, exclude = lists_for(self.schema)
        self.exprs, self.tags = R.make_expressions(E, 7, rng)
        self.exp = R.Expectation(self.exprs, self.tags, {}, self.schema, include, exclude)
        self.valid = TE.valid_fields(self.schema, include, exclude)
        self.records = TE.planted_records(N, self.schema, rng, self.valid)
        texts, self.field, self.rec_off = R.csr(self.records, self.schema)
        self.hits = self.exp.hit_bitmap(texts)
        self.E, self.expr_tag = E, tag_ids(self.tags)
        self.g = make_group(self.exprs, self.tags, self.schema, include, exclude)

    def want(self, hits=None, field=None, rec_off=None):
        return TE.expected(self.hits if hits is None else hits, self.E, self.field if field is None else field,
                           self.rec_off if rec_off is None else rec_off, self.valid)


_cases = {}


def case(E, F, **kw):
    key = (E, F, tuple(sorted(kw.items())))
    if key not in _cases:
        _cases[key] = Case(E, F, **kw)
    return _cases[key]


# ---- 1. word borders of the hit rows and of the validity mask -------------------------------------------------------------
@pytest.mark.parametrize("E", [1, 31, 32, 33, 64, 65, 2049, 4097])
def test_expression_counts_at_the_word_borders(E):
    c = case(E, 8)
    want = c.want()
    TE.assert_not_vacuous(want[3])
    TE.assert_entries(c.g.debug_tag_entries(c.hits, E, c.field, c.rec_off), want, c.expr_tag)
    assert c.g.tags_from_entries(*want[:3]) == TE.tag_maps(c.exp, c.records, c.hits)


@pytest.mark.parametrize("F", [1, 32, 33, 65])
def test_field_counts_with_excluded_fields_at_31_and_32(F):
    c = case(40, F)
    if F > 32:
        # (an excluded path is a prefix: "G8" at index 32 takes "G8.a" ... behind it along)
        assert not c.valid[31] and not c.valid[32] and c.valid[30] and (F == 33 or any(c.valid[33:]))
    want = c.want()
    TE.assert_not_vacuous(want[3], masked=F > 1)          # (one field: nothing can be excluded beside it)
    TE.assert_entries(c.g.debug_tag_entries(c.hits, 40, c.field, c.rec_off), want, c.expr_tag)
    assert c.g.tags_from_entries(*want[:3]) == TE.tag_maps(c.exp, c.records, c.hits)


@pytest.mark.parametrize("include,exclude", [(["G"], ["G0."]), (["G1", "G0"], ["G0"]), (["G0.a"], ["G0.a"]), (["G2"], ["G"])])
def test_include_and_exclude_overlap_exclude_wins(include, exclude):
    c = case(40, 12, include=tuple(include), exclude=tuple(exclude), lists=False)
    want = c.want()
    if any(c.valid):
        TE.assert_not_vacuous(want[3])
    else:
        assert want[3]["total"] == 0 and want[3]["masked"] > 0               # all leaves invalid: hits, and not one entry
    TE.assert_entries(c.g.debug_tag_entries(c.hits, 40, c.field, c.rec_off), want, c.expr_tag)


# ---- 2. shapes ---------------------------------------------------------------------------------------------------------------
def test_empty_records_first_middle_and_last():
    c = case(40, 8)
    sizes = np.diff(c.rec_off.astype(np.int64))
    assert sizes[0] == 0 and sizes[-1] == 0 and (sizes[1:-1] == 0).any() and (sizes > 0).any()
    got = c.g.debug_tag_entries(c.hits, 40, c.field, c.rec_off)
    assert got[0][0] == 0 and got[0][1] == 0 and got[0][-1] == got[0][-2] == got[4]


def test_no_records_and_no_leaves():
    c = case(40, 8)
    row_off, ef, ee, et, total = c.g.debug_tag_entries(c.hits[:0], 40, [], [0])
    assert total == 0 and [int(x) for x in row_off] == [0] and (ef == TE.GUARD_HOST).all()
    row_off, ef, ee, et, total = c.g.debug_tag_entries(c.hits[:0], 40, [], [0, 0, 0])
    assert total == 0 and [int(x) for x in row_off] == [0, 0, 0]
    with pytest.raises(group.GroupFinderError) as ei:
        c.g.debug_tag_entries(c.hits[:1], 40, [0], [1])                      # leaves but no records
    assert ei.value.code == _lib.GFT_E_INVALID and "no records" in str(ei.value)


def test_a_repeated_field_contributes_twice_and_the_map_drops_the_duplicate():
    c = case(40, 8)
    p = c.schema[0]
    recs = [[(p, TE.EVERYTHING), (p, TE.EVERYTHING), (c.schema[1], "")], [(p, R.A)]]
    texts, field, rec_off = R.csr(recs, c.schema)
    hits = c.exp.hit_bitmap(texts)
    want = c.want(hits, field, rec_off)
    k = int(want[0][1]) // 2
    assert k > 0 and want[3]["silent"] == 1 and np.array_equal(want[2][:k], want[2][k:2 * k])      # the same leaf twice: the same entries twice
    got = c.g.debug_tag_entries(hits, 40, field, rec_off)
    TE.assert_entries(got, want, c.expr_tag)
    once = c.g.tags_from_entries(*c.want(hits[[0, 3]], field[[0, 3]], np.asarray([0, 1, 2], np.uint64))[:3])
    assert c.g.tags_from_entries(got[0], got[1][:got[4]], got[2][:got[4]]) == once


@pytest.mark.parametrize("E", [33, 64, 65, 2049])
def test_dense_rows_and_garbage_above_the_last_expression(E):
    c = case(E, 8)
    dense = np.full_like(c.hits, 0xFFFFFFFF)                               # every bit set, those at and above E included
    want = c.want(dense)
    n_valid_leaves = sum(c.valid[int(f)] for f in c.field)
    assert want[3]["total"] == E * n_valid_leaves and 0 < n_valid_leaves < len(c.field)
    TE.assert_entries(c.g.debug_tag_entries(dense, E, c.field, c.rec_off), want, c.expr_tag)
    dirty = c.hits.copy()                                                   # the oracle's rows with garbage above E
    if E % 32:
        dirty[:, -1] |= np.uint32((0xFFFFFFFF << (E % 32)) & 0xFFFFFFFF)
        assert not np.array_equal(dirty, c.hits)
    TE.assert_entries(c.g.debug_tag_entries(dirty, E, c.field, c.rec_off), c.want(), c.expr_tag)


def test_a_finder_without_expressions_and_a_group_without_rules():
    g = make_group([], [], ["Field", "Other"])
    row_off, ef, ee, et, total = g.debug_tag_entries(np.zeros((3, 0), np.uint32), 0, [0, 1, 0], [0, 1, 3])
    assert total == 0 and [int(x) for x in row_off] == [0, 0, 0]
    assert g.tags_from_entries(row_off, ef[:0], ee[:0]) == [{}, {}]
    c = case(40, 8)
    assert c.g.rule_exprs() == []                                           # (every Case is a group without rules)


# ---- 3. the cap protocol -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [40, 2049])
def test_caps_store_a_prefix_and_nothing_behind_it(E):
    c = case(E, 8)
    want = c.want()
    total = want[3]["total"]
    assert total > 8
    for cap in (0, 1, total - 1, total, total + 7):
        for want_tag in (True, False):
            TE.assert_entries(c.g.debug_tag_entries(c.hits, E, c.field, c.rec_off, cap=cap, want_tag=want_tag), want, c.expr_tag, cap=cap)
    # NULL arrays with cap == 0 count only
    L = _lib.load()
    import ctypes as C
    row_off, t = np.zeros(len(c.rec_off), np.uint64), C.c_uint64()
    assert L.gft_debug_tag_entries(c.g._h, c.hits.ctypes.data, E, c.field.ctypes.data, c.rec_off.ctypes.data, len(c.rec_off) - 1, len(c.field),
                                   row_off.ctypes.data, None, None, None, 0, C.byref(t)) == 0
    assert t.value == total and np.array_equal(row_off, want[0])
    assert L.gft_debug_tag_entries(c.g._h, c.hits.ctypes.data, E, c.field.ctypes.data, c.rec_off.ctypes.data, len(c.rec_off) - 1, len(c.field),
                                   row_off.ctypes.data, None, None, None, 5, C.byref(t)) == _lib.GFT_E_INVALID


# ---- 4. validation -------------------------------------------------------------------------------------------------------------
def test_validation_refusals_leave_the_handle_usable():
    c = case(40, 8)
    n = len(c.field)
    bad_field = c.field.copy()
    bad_field[n // 2] = len(c.schema)                                       # a field index equal to n_fields
    bad_off = c.rec_off.copy()
    k = int(np.flatnonzero(np.diff(c.rec_off.astype(np.int64)) > 0)[0])
    bad_off[k], bad_off[k + 1] = bad_off[k + 1], bad_off[k]                 # descending
    short = c.rec_off.copy()
    short[-1] += 1
    for field, rec_off, word in [(bad_field, c.rec_off, "field"), (c.field, bad_off, "descends"), (c.field, short, "n_leaves")]:
        with pytest.raises(group.GroupFinderError) as ei:
            c.g.debug_tag_entries(c.hits, 40, field, rec_off)
        assert ei.value.code == _lib.GFT_E_INVALID and word in str(ei.value)
        with pytest.raises(group.GroupFinderError) as ei:                   # the host-pointer call checks the same things first
            c.g.TagRecordsEntries(np.zeros(64, np.uint8), np.zeros(n + 1, np.uint64), field, rec_off)
        assert ei.value.code == _lib.GFT_E_INVALID and word in str(ei.value)
    with pytest.raises(group.GroupFinderError) as ei:
        c.g.debug_tag_entries(c.hits, 41, c.field, c.rec_off)               # not the finder's number of expressions
    assert ei.value.code == _lib.GFT_E_INVALID
    f = Finder(None, None, False, allow_no_device=True)
    with pytest.raises(group.GroupFinderError) as ei:
        group.NewFinder(f).debug_tag_entries(np.zeros((1, 0), np.uint32), 0, [0], [0, 1])
    assert ei.value.code == _lib.GFT_E_INVALID and "schema" in str(ei.value)
    TE.assert_entries(c.g.debug_tag_entries(c.hits, 40, c.field, c.rec_off), c.want(), c.expr_tag)


# ---- 5. the tag map ------------------------------------------------------------------------------------------------------------
def test_tags_from_entries_is_tag_object_for_objects_with_unique_fields():
    rng = np.random.default_rng(21)
    V = R.vocabulary()
    exprs, tags = R.make_expressions(40, 5, rng)

    def text():
        return " ".join(V[int(x)] for x in rng.integers(0, len(V), int(rng.integers(0, 6))))
    objs = [{"Body": text(), "Meta": {"Notes": text(), "Tags": [text(), text(), {"Deep": text()}]}, "n": 3, "Skip": {"x": text()}, "": text()}
            for _ in range(30)] + [{}, {"Body": ""}, "top-level string " + V[0], [text(), [text()]]]
    schema = list(dict.fromkeys(p for o in objs for p, _ in R.flatten(o)))
    include, exclude = ["Body", "Meta", "index", ""], ["Meta.Tags.index(1)", "Skip"]
    exp = R.Expectation(exprs, tags, {}, schema, include, exclude)
    ref = group_ref.GroupFinder(lambda t: [(tags[i], exprs[i]) for i in range(40) if int(exp.hit_bitmap([t])[0, i >> 5]) >> (i & 31) & 1])
    recs = [R.flatten(o) for o in objs]
    assert all(len({p for p, _ in rec}) == len(rec) for rec in recs)        # unique fields
    texts, field, rec_off = R.csr(recs, schema)
    hits = exp.hit_bitmap(texts)
    g = make_group(exprs, tags, schema, include, exclude)
    row_off, ef, ee, et, total = g.debug_tag_entries(hits, 40, field, rec_off)
    want = TE.expected(hits, 40, field, rec_off, TE.valid_fields(schema, include, exclude))
    TE.assert_not_vacuous(want[3])
    TE.assert_entries((row_off, ef, ee, et, total), want, tag_ids(tags))
    got = g.tags_from_entries(row_off, ef[:total], ee[:total])
    assert got == [{t: {f: sorted(v) for f, v in fs.items()} for t, fs in ref.tag_object(o, include, exclude).items()} for o in objs]
    assert sum(len(m) for m in got) > 0


def test_tag_records_of_a_regex_finder_takes_the_host_route():
    """A finder with a regex term never qualifies for the device route: gft_group_tag_records gets the leaf bitmap from
    Finder::ProcessTexts and makes the entries with tag_entries_host.  ProcessTexts solves on the device, so on a box without one
    a batch with leaves ends in the finder's "no HIP device" -- the call's error, after which the handle answers; where there is a
    device the maps are compared with the oracle (tests/test_gpu_tags.py does the same under the gpu mark)."""
    rng = np.random.default_rng(22)
    schema = R.make_schema(8)
    exprs, tags = R.make_expressions(40, 5, rng)
    exclude = [schema[2]]
    exp = R.Expectation(exprs, tags, {}, schema, None, exclude)
    g = make_group(exprs + [r'r"zq+x[0-9]"'], tags + ["rxtag"], schema, None, exclude, rgx=PyRegexpEngine())
    assert g.findthem.GetRegexes()
    assert g.TagRecords([[], []]) == [{}, {}]                               # no leaves: no finder call, the host route answers
    recs = TE.planted_records(30, schema, rng, TE.valid_fields(schema, None, exclude))
    try:
        got = g.TagRecords(recs)
    except group.GroupFinderError as e:
        if "no HIP device" not in str(e):
            raise
        assert g.TagRecords([[]]) == [{}]
        return
    want = TE.tag_maps(exp, recs)                                           # (the regex never matches: "rxtag" tags nothing)
    assert got == want and sum(len(m) for m in want) > 0


# ---- 6. the C ABI ----------------------------------------------------------------------------------------------------------------
def test_symbols_of_the_tag_calls_are_exported_and_declared():
    L = _lib.load()
    hdr = open(os.path.join(os.path.dirname(_lib.HERE), "include", "gft.h")).read()
    for name in ("gft_group_tag_records_device", "gft_group_tag_records", "gft_group_tag_jsons_device", "gft_group_tag_jsons_schema",
                 "gft_group_tag_jsons_auto", "gft_debug_tag_entries", "gft_debug_tag_entries_device"):
        assert hasattr(L, name) and name in _lib.SYMBOLS and ("int %s(" % name) in hdr
