"""The inputs of tests/schema_scale.py without a device: every JSON case through the host emulation of the walker
(gft_debug_emulate_json_leaves) and through gft_debug_json_leaves_ref, every rule case through the host interpreter
(gft_debug_eval_rules) and through oracle/group_ref.py's evaluate_rules.  What the kernels must give in test_gpu_schema_scale.py
is pinned here, so that a difference there belongs to the device; and the conditions on the generators are asserted here,
over all cases, whichever tests were selected.  Nothing here needs a GPU."""
import json
import re

import numpy as np
import pytest

import json_docs as J
import records as R
import schema_scale as S
from gofindthem_amd import _lib, finder, group

_GROUPS = {}


def json_group(schema):
    if schema not in _GROUPS:
        f = finder.Finder(None, None, False, allow_no_device=True)
        g = group.NewFinderWithRules(f, {})
        g.SetSchema(S.SCHEMAS[schema])
        g._keep = f
        _GROUPS[schema] = g
    return _GROUPS[schema]


_JSON = {}


def json_result(case):
    """the reference's arrays of a case, the emulation checked against them (once per session)"""
    if case.name not in _JSON:
        g = json_group(case.schema)
        ref = g.debug_json_leaves_ref(case.docs)
        S.same_leaves(g.debug_emulate_json_leaves(case.docs), ref)
        _JSON[case.name] = ref
    return _JSON[case.name]


@pytest.mark.parametrize("name", S.JSON_CASES)
def test_json_case_walker_equals_reference(name):
    case = S.JSON_CASES[name]()
    ref = json_result(case)
    if case.want is not None:
        assert [int(s) for s in ref[0]] == case.want
    if case.fields is not None:
        assert [int(f) for f in ref[2][:ref[5][0]]] == case.fields


def test_json_cases_under_caps():
    case = S.corpus()
    g = json_group(case.schema)
    n_leaves, n_text = json_result(case)[5]
    for caps in ((n_leaves - 1, n_text - 1), (3, n_text)):
        S.same_leaves(g.debug_emulate_json_leaves(case.docs, *caps), g.debug_json_leaves_ref(case.docs, *caps))


def test_wide_cover_reads_every_key_once():
    case = S.wide_cover()
    assert len(case.docs) == 256 + 3 and sorted(case.fields) == list(range(16383))
    got = J.leaves_of(*json_result(case)[:5])
    assert got[0][1][0] == (case.fields[0], b"v%d" % case.fields[0]) and [len(x[1]) for x in got[:256]] == [64] * 255 + [63]


def test_long_keys_cross_the_piece_borders_at_different_lanes():
    case = S.long_keys()
    starts = {(d.index(b'{"n":{"') + 8 if b'{"n":' in d[:80] else d.index(b'"') + 1) % 64 for d in case.docs}
    assert starts == {2, 3, 39, 1, 8, 9, 45, 7}                    # (0, 1, 37, 63 spaces and '{"' or '{"n":{"' in front of the key)
    assert len(case.fields) == len(S.KEY_LENGTHS) * 8 and S.SCHEMAS["long keys"][case.fields[-1]] == "n." + S.LONG_KEY[65535]


def test_indices_give_their_leaves_in_order():
    got = J.leaves_of(*json_result(S.indices())[:5])
    assert got[0] == (0, [(i, b"s%d" % k) for i, k in enumerate(S.INDEX_AT)]) and got[2] == (0, [(9, b"deep")])
    assert got[8] == (0, [(2, b"s10"), (5, b"s100")])


def test_tiled_batch_strides_and_is_not_periodic():
    case = S.tiled(256)
    assert len(case.docs) == S.tiled_count(256) > 2 * 32 * 256
    per_wave = [sum(1 for c in case.clean[w::32 * 256] if not c) for w in range(0, 32 * 256, 257)]
    assert len(set(per_wave)) > 1


def test_write_pass_order_is_what_it_says():
    case = S.write_pass_order()
    ref = json_result(case)
    n = np.diff(ref[1].astype(np.int64))
    for k in range(0, len(case.docs), 192):
        assert ref[0][k:k + 64].all() and not ref[0][k + 64:k + 192].any()
        assert not n[k:k + 128].any() and n[k + 128:k + 192].sum() > 64
    assert {J.SYNTAX, J.DEPTH, J.PATH, J.KEY, J.DUP, J.TEXT} <= {int(s) for s in ref[0]}


def test_json_generators_are_not_one_sided():
    """in every JSON case that mixes clean and broken documents the clean ones have status 0 under the reference, at least 10 % of
    the batch has another status, and the batch yields leaves.  Always over all cases."""
    mixed = [c for c in (make() for make in S.JSON_CASES.values()) if c.clean is not None]
    assert len(mixed) >= 6
    for case in mixed:
        ref = json_result(case)
        bad = [case.docs[i][:80] for i in range(len(case.docs)) if case.clean[i] and ref[0][i] != 0]
        assert not bad, (case, bad[:3])
        assert int((ref[0] != 0).sum()) >= 0.10 * len(case.docs), (case, int((ref[0] != 0).sum()))
        assert ref[5][0] > 0, case


def test_strided_reset_documents_reach_the_last_words():
    case = S.strided_reset()
    ref = json_result(case)
    assert len(case.docs) >= 500 and all(b'"p16000"' in d for d in case.docs)
    assert [int(s) for s in ref[0]] == [J.OK if c else J.DUP for c in case.clean]
    fields = ref[2][:ref[5][0]]
    assert int((fields >= 2048).sum()) > 10 * len(case.docs) // 2 and int((fields < 2048).sum()) > 100


def test_end_to_end_documents():
    exprs, tags, rules, docs, broken, clean = S.end_to_end()
    g = json_group("nested")
    ref = g.debug_json_leaves_ref(docs)
    assert len(docs) == 300 and not ref[0].any() and ref[5][0] > 300 * 50
    S.same_leaves(g.debug_emulate_json_leaves(docs), ref)
    assert J.leaves_of(*ref[:5])[5][1] == [(S.NESTED.index(p), t.encode("utf-8")) for p, t in R.flatten(json.loads(docs[5].decode("utf-8")))]
    ref = g.debug_json_leaves_ref(broken)
    S.same_leaves(g.debug_emulate_json_leaves(broken), ref)
    assert not any(ref[0][i] for i in range(len(broken)) if clean[i]) and int((ref[0] != 0).sum()) >= 0.10 * len(broken)


# ---- rules --------------------------------------------------------------------------------------------------------------
_checked = set()


def rule_group(case):
    f = finder.Finder(None, None, False, allow_no_device=True)
    for e, t in zip(case.exprs, case.tags):
        f.AddExpressionWithTag(e, t)
    g = group.NewFinderWithRules(f, case.rules)
    g.SetSchema(case.schema, case.include, case.exclude)
    return g


def rule_check(case):
    """gft_debug_eval_rules over the case's bitmap, clean and with garbage above the last expression == the oracle's rows"""
    if case.name not in _checked:
        g = rule_group(case)
        assert g.rule_exprs() == case.exp.numbering
        for hits in (case.hits, case.dirty_hits()):
            assert np.array_equal(g.debug_eval_rules(hits, len(case.exprs), case.field, case.rec_off), case.want)
        _checked.add(case.name)
    return case


@pytest.mark.parametrize("name", S.RULE_CASES)
def test_rule_case_interpreter_equals_oracle(name):
    rule_check(S.RULE_CASES[name]())


def test_rule_case_shapes():
    for n in S.UNIT_COUNTS:
        case = S.unit_case(n)
        units = {u for _, raw in case.exp.numbering for u in re.findall(r'"([^"]*)"', raw)}
        assert len(units) == n and len(case.exp.numbering) == (n + 7) // 8
        sizes = sorted(len(r) for r in case.records)
        assert len(sizes) == 130 and sizes[-2:] == [257, 600] and sizes[0] == 0 and sizes[-3] <= 40
    deep = S.unit_case(8192, deep=8)
    assert len(deep.exp.numbering) == 1024 + 8 and len(deep.high_unit_columns()) >= 1024 - 32
    # nested_rule(.., d) needs a stack of exactly d: 32 compiles (the cases above), 33 is refused by name
    small = S.depth_case(32)
    g = rule_group(small)
    g.AddRule("too_deep", [S.nested_rule(["tag0:G0", "tag1"], 33, np.random.default_rng(0))])
    with pytest.raises(group.GroupFinderError) as ei:
        g.debug_eval_rules(small.hits, len(small.exprs), small.field, small.rec_off)
    assert ei.value.code == _lib.GFT_E_UNSUPPORTED and "stack of 33" in str(ei.value)
    chunks = S.chunks_case()
    sizes = [len(r) for r in chunks.records]
    assert sizes[:64] == [300] * 64 and sizes[128:133] == [256, 257, 300, 0, 300] and sum(sizes[64:128]) % 256 == 64
    a, b = 64 * 300, 64 * 300 + sum(sizes[64:128])
    assert not chunks.hits[a:b - 1].any() and chunks.hits[b - 1].any()
    # (record 131 is empty; 64..126 have leaves without a tag; 127 ends with the one tagged leaf)
    assert all(np.array_equal(chunks.want[r], chunks.want[131]) for r in range(64, 127)) and not np.array_equal(chunks.want[127], chunks.want[131])
    big = S.field_words_case()
    assert len(big.schema) == 65535 and {0, 1, 255, 256, 65534, 65311, 65312} <= {int(f) for f in big.field}
    four = S.four_words_case()
    assert len(four.exprs) == 100 and len(set(four.tags)) == 97 and not np.array_equal(four.dirty_hits(), four.hits)


def test_rule_generators_are_not_one_sided():
    """conditions on the generators, not tolerances.  In every rule case between 10 % and 90 % of the (record, rule expression)
    answers are true; in the unit-count cases also among the expressions whose units all have an index of 256 or more; with
    65 535 fields at least 10 % of the (record, UNIT with a path) pairs whose tag the record carries carry it only outside the
    prefix -- answers that the field masks decide.  Always over all cases."""
    for make in S.RULE_CASES.values():
        case = rule_check(make())
        true, total = case.true_share()
        assert 0.10 * total <= true <= 0.90 * total, (case, true, total)
    for case in [S.unit_case(n) for n in S.UNIT_COUNTS] + [S.unit_case(8192, deep=8)]:
        columns = case.high_unit_columns()
        assert bool(columns) == (len(case.exp.numbering) > 32), case
        if columns:
            true, total = case.true_share(columns)
            assert 0.10 * total <= true <= 0.90 * total, (case, true, total)
    for case in (S.field_words_case(), S.include_exclude_case()):
        present, outside = case.exp.prefix_dependence(case.maps)
        assert outside >= 0.10 * present > 0, (case, outside, present)


def test_a_field_index_at_the_schema_size_is_refused():
    case = S.field_words_case()
    g = rule_group(case)
    field = case.field.copy()
    field[len(field) // 2] = 65535
    with pytest.raises(group.GroupFinderError) as ei:
        g.debug_eval_rules(case.hits, len(case.exprs), field, case.rec_off)
    assert ei.value.code == _lib.GFT_E_INVALID and "field" in str(ei.value)
    assert np.array_equal(g.debug_eval_rules(case.hits, len(case.exprs), case.field, case.rec_off), case.want)
