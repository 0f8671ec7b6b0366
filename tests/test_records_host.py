"""The record form of the group finder, host half: the rule compiler (csrc/rule_set.cpp) and its device words -- field masks,
units, postfix programs -- interpreted by gft_debug_eval_rules over leaf bitmaps taken from the CPU oracle, against
oracle/group_ref.py's evaluate_rules (tests/records.py).  Nothing here needs a GPU."""
import numpy as np
import pytest

import records as R
from conftest import load_golden
from gofindthem_amd import _lib, group
from gofindthem_amd.finder import Finder

FIX = load_golden("group_finder.json")


def make_group(exprs, tags, rules, schema=None, include=None, exclude=None):
    f = Finder(None, None, False, allow_no_device=True)
    for e, t in zip(exprs, tags):
        f.AddExpressionWithTag(e, t)
    g = group.NewFinderWithRules(f, rules)
    if schema is not None:
        g.SetSchema(schema, include, exclude)
    return g


def check(g, exp, records, hits=None):
    """gft_debug_eval_rules over the oracle's leaf bitmap == the oracle's rule rows; returns the rule dicts"""
    texts, field, rec_off = R.csr(records, exp.schema)
    if hits is None:
        hits = exp.hit_bitmap(texts)
    want, _ = exp.rules_of(records, hits)
    got = g.debug_eval_rules(hits, len(exp.exprs), field, rec_off)
    assert g.rule_exprs() == exp.numbering
    assert np.array_equal(got, exp.bitmap_of(want))
    assert g.rules_from_bitmap(got) == want
    return want


# ---- 1. the reference's own group fixtures, flattened to records --------------------------------------------------------
def test_example_program_object_as_a_record():
    ex = FIX["example"]
    exprs = [(e, tag) for tag, es in ex["finder_rules"].items() for e in es]
    obj_leaves = R.flatten(ex["object"])
    arr_leaves = R.flatten(ex["array"])
    schema = list(dict.fromkeys(p for p, _ in obj_leaves + arr_leaves))
    for include, records, want in [(["Field3", "Field3.SomeField1"], [obj_leaves], ex["expected_rules_with_field_names"]),
                                   (None, [arr_leaves], ex["expected_array_rules"])]:
        exp = R.Expectation([e for e, _ in exprs], [t for _, t in exprs], ex["rules"], schema, include, None)
        assert not ex["case_sensitive"]
        g = make_group(exp.exprs, exp.tags, ex["rules"], schema, include)
        assert check(g, exp, records) == [want]


def test_tag_object_cases_as_records():
    sec = FIX["tag_object"]
    assert not sec["case_sensitive"]
    exprs = [x["expression"] for x in sec["finder_expressions"]]
    tags = [x["tag"] for x in sec["finder_expressions"]]
    n = 0
    for c in sec["cases"]:
        if c.get("struct"):
            continue                      # (unexported struct fields are the walk's business, not the record form's)
        leaves = R.flatten(c["object"])
        schema = list(dict.fromkeys(p for p, _ in leaves)) or ["x"]
        exp = R.Expectation(exprs, tags, sec["rules"], schema)
        g = make_group(exprs, tags, sec["rules"], schema)
        want = check(g, exp, [leaves])
        _, maps = exp.rules_of([leaves])
        assert {t: {f: sorted(v) for f, v in fs.items()} for t, fs in maps[0].items()} == c["expected"], c["message"]
        assert want == [exp.ref.evaluate_rules(c["expected"])]
        n += 1
    assert n > 0


# ---- 2. named rows ----------------------------------------------------------------------------------------------------
A, B = R.A, R.B


@pytest.mark.parametrize("row", R.named_rows(), ids=lambda r: r[0])
def test_named_rows(row):
    _, exprs, tags, rules, schema, inc, exc, recs, want = row
    exp = R.Expectation(exprs, tags, rules, schema, inc, exc)
    g = make_group(exprs, tags, rules, schema, inc, exc)
    assert check(g, exp, recs) == want


# ---- 3. random batches against the oracle -----------------------------------------------------------------------------
FAMILY = [(seed, F, T, Rn) for seed in range(3) for F in (1, 32, 33, 65) for T in (1, 33) for Rn in (1, 32, 33, 65)]
_results = {}


def family_case(seed, F, T, Rn, N=96):
    rng = np.random.default_rng([seed, F, T, Rn])
    schema = R.make_schema(F)
    exprs, tags = R.make_expressions(max(T, 40), T, rng)
    rules = R.make_rules(Rn, T, schema, rng)
    inc, exc = [(None, None), (None, [schema[-1]]), (["G"], [schema[0] + "."])][seed]
    return exprs, tags, rules, schema, inc, exc, R.make_records(N, schema, rng)


def family_result(case):
    """checks one case against the oracle (once per session) -> (true answers, all answers, (record, UNIT with a path) pairs whose
    tag the record carries, those of them that carry it only outside the prefix)"""
    if case not in _results:
        exprs, tags, rules, schema, inc, exc, recs = family_case(*case)
        exp = R.Expectation(exprs, tags, rules, schema, inc, exc)
        g = make_group(exprs, tags, rules, schema, inc, exc)
        texts, _, _ = R.csr(recs, schema)
        hits = exp.hit_bitmap(texts)
        want = check(g, exp, recs, hits)
        _, maps = exp.rules_of(recs, hits)
        present, outside = exp.prefix_dependence(maps)
        _results[case] = (sum(len(v) for d in want for v in d.values()), len(recs) * len(exp.numbering), present, outside)
    return _results[case]


@pytest.mark.parametrize("seed,F,T,Rn", FAMILY)
def test_random_batches_match_the_oracle(seed, F, T, Rn):
    family_result((seed, F, T, Rn))


def test_random_families_are_not_one_sided():
    """conditions on the generator, not tolerances: over every family (all cases that share an F, a T, an R or a seed) at least
    10 % of the (record, rule expression) answers are true and at least 10 % false, and of the (record, UNIT with a field
    path) pairs whose tag the record carries at least 10 % carry it only outside the prefix -- answers the masks decide.
    Always over the whole FAMILY, whichever tests were selected."""
    totals = {}
    for case in FAMILY:
        res = family_result(case)
        for key in zip(("seed", "F", "T", "R"), case):
            t = totals.setdefault(key, [0, 0, 0, 0])
            for k in range(4):
                t[k] += res[k]
    assert len(totals) == 3 + 4 + 2 + 4
    for key, (true, total, present, outside) in sorted(totals.items()):
        assert 0.10 * total <= true <= 0.90 * total, (key, true, total)
        assert outside >= 0.10 * present > 0, (key, outside, present)


# ---- 4. limits and numbering -------------------------------------------------------------------------------------------
def _status(fn, *a):
    with pytest.raises(group.GroupFinderError) as ei:
        fn(*a)
    return ei.value.code, str(ei.value)


def test_unit_limit_8192_passes_8193_is_refused():
    schema = ["f%d" % i for i in range(128)]
    exprs, tags = ['"%s"' % A] * 64, ["tag%d" % t for t in range(64)]
    units = ['"tag%d:f%d"' % (t, i) for t in range(64) for i in range(128)]              # 8192 distinct (tag, field path) pairs
    rules = {"r": [" or ".join(units[k:k + 64]) for k in range(0, 8192, 64)]}
    g = make_group(exprs, tags, rules, schema)
    exp = R.Expectation(exprs, tags, rules, schema)
    recs = [[("f5", A)], [("f70", A), ("f5", B)], []]
    want = check(g, exp, recs)
    assert [len(d.get("r", ())) for d in want] == [64, 128, 0]          # "f5" lies in every tag's first chunk, "f7" and "f70" in both
    g.AddRule("s", ['"tag0:f5" or "one_more:f5"'])                                        # an unknown tag is a unit of its own
    texts, field, rec_off = R.csr(recs, schema)
    code, msg = _status(g.debug_eval_rules, exp.hit_bitmap(texts), 64, field, rec_off)
    assert code == _lib.GFT_E_UNSUPPORTED and "8192" in msg
    # the handle is still usable: the schema call is refused the same way, other entry points answer
    code, msg = _status(g.SetSchema, schema)
    assert code == _lib.GFT_E_UNSUPPORTED and "8192" in msg
    assert g.EvaluateRules({"tag0": {"f5": [A]}})["s"] == ['"tag0:f5" or "one_more:f5"']


def _nested(depth):
    """a right-nested chain whose postfix program needs an operand stack of exactly `depth`"""
    s = '"tag0"'
    for _ in range(depth - 1):
        s = '"tag1" or (%s)' % s
    return s


def test_depth_32_passes_33_is_refused_and_the_previous_set_still_answers():
    e2, t2 = ['"%s"' % A, '"%s"' % B], ["tag0", "tag1"]
    schema = ["Field", "Other"]
    rules = {"deep": [_nested(32)], "flat": ['not "tag1:Other"']}
    exp = R.Expectation(e2, t2, rules, schema)
    g = make_group(e2, t2, rules, schema)
    recs = [[("Field", A)], [("Other", B)], [], [("Field", "")]]
    want = check(g, exp, recs)
    assert want == [{"deep": [_nested(32)], "flat": ['not "tag1:Other"']}, {"deep": [_nested(32)]}, {"flat": ['not "tag1:Other"']},
                    {"flat": ['not "tag1:Other"']}]
    # a schema the compiler refuses leaves the previous schema and its set answering
    code, msg = _status(g.SetSchema, ["p%d" % i for i in range(65536)])
    assert code == _lib.GFT_E_UNSUPPORTED and "65535" in msg
    code, msg = _status(g.SetSchema, ["twice", "twice"])
    assert code == _lib.GFT_E_INVALID
    assert check(g, exp, recs) == want
    g.SetSchema(["p%d" % i for i in range(65535)])
    g.SetSchema(schema)
    # a rule the compiler refuses: the record calls say which limit, the handle keeps working
    g.AddRule("too_deep", [_nested(33)])
    texts, field, rec_off = R.csr(recs, schema)
    code, msg = _status(g.debug_eval_rules, exp.hit_bitmap(texts), 2, field, rec_off)
    assert code == _lib.GFT_E_UNSUPPORTED and "32" in msg and "too_deep" in msg
    assert g.EvaluateRules({"tag0": {"Field": [A]}})["too_deep"] == [_nested(33)]


def test_numbering_is_sorted_rule_names_then_insertion_order():
    e2, t2 = ['"%s"' % A], ["tag0"]
    g = make_group(e2, t2, {}, ["Field"])
    assert g.rule_exprs() == [] and g.rule_words() == 0
    assert g.debug_eval_rules(np.zeros((1, 1), np.uint32), 1, [0], [0, 1]).shape == (1, 0)      # a group without rules is valid
    for name, e in [("zeta", '"tag0"'), ("alpha", 'not "tag0"'), ("zeta", '"tag0:Field"'), ("Beta", '"tag0" or "x"'), ("alpha", '"tag0"'),
                    ("é", '"tag0"')]:
        g.AddRule(name, [e])
    want = [("Beta", '"tag0" or "x"'), ("alpha", 'not "tag0"'), ("alpha", '"tag0"'), ("zeta", '"tag0"'), ("zeta", '"tag0:Field"'), ("é", '"tag0"')]
    assert g.rule_exprs() == want
    got = g.debug_eval_rules(np.asarray([[1]], np.uint32), 1, [0], [0, 1, 1])
    assert [int(x) for x in got[:, 0]] == [0b111101, 0b000010]


# ---- 5. validation ---------------------------------------------------------------------------------------------------
def test_validation_refusals_leave_the_handle_usable():
    e2, t2 = ['"%s"' % A], ["tag0"]
    g = make_group(e2, t2, {"r": ['"tag0"']})
    hit = np.asarray([[1], [0]], np.uint32)
    code, msg = _status(g.debug_eval_rules, hit, 1, [0, 0], [0, 1, 2])
    assert code == _lib.GFT_E_INVALID and "schema" in msg
    g.SetSchema(["Field", "Other"])
    for field, rec_off, word in [([0, 2], [0, 1, 2], "field"), ([0, 1], [0, 2, 1], "descends"), ([0, 1], [0, 1, 1], "n_leaves"),
                                 ([0, 1], [0, 1, 3], "n_leaves")]:
        code, msg = _status(g.debug_eval_rules, hit, 1, field, rec_off)
        assert code == _lib.GFT_E_INVALID and word in msg, msg
    code, msg = _status(g.debug_eval_rules, hit, 2, [0, 1], [0, 1, 2])
    assert code == _lib.GFT_E_INVALID
    code, msg = _status(g.debug_eval_rules, hit, 1, [0, 1], [2])              # leaves but no records
    assert code == _lib.GFT_E_INVALID and "no records" in msg
    g0 = make_group(e2, t2, {}, ["Field", "Other"])                             # a group without rules checks its batches all the same
    code, msg = _status(g0.debug_eval_rules, hit, 1, [0, 2], [0, 1, 2])
    assert code == _lib.GFT_E_INVALID and "field" in msg
    assert g0.debug_eval_rules(hit, 1, [0, 1], [0, 1, 2]).shape == (2, 0)
    # garbage above the last expression's bit is not read
    assert [int(x) for x in g.debug_eval_rules(hit | np.uint32(0xFFFFFFFE), 1, [0, 1], [0, 1, 2])[:, 0]] == [1, 0]
    assert g.debug_eval_rules(hit[:0], 1, [], [0]).shape == (0, 1)
    assert [int(x) for x in g.debug_eval_rules(hit[:0], 1, [], [0, 0])[:, 0]] == [0]
