"""The group finder's device kernels at the size of a production schema (inputs: tests/schema_scale.py; the same inputs
through the host walker and the host interpreter: test_schema_scale_host.py).

k_json (csrc/gft_json.hip) against gft_debug_json_leaves_ref in every array: with the engine held to one CU, so that each of
its 32 waves walks tens to hundreds of documents in a row -- broken ones in front of clean ones, under caps, the write pass
skipping --; on the default grid with more than two documents per wave; over a trie at the node limit, where the reset of the
visited bitset strides; keys of 63 to 65 535 bytes and their near misses; array indices of up to four digits.

k_leaf_tags and k_record_rules (csrc/gft_rules.hip) over a caller-supplied leaf bitmap (gft_debug_eval_rules_device) against
oracle/group_ref.py's evaluate_rules: 255 to 8 192 units, operand stacks of 31 and 32 (with 8 192 units the 135 696-byte
launch), 65 535 fields, four words of tags and of expressions, records of 256 to 600 leaves.

Every comparison is bit for bit."""
import contextlib
import json

import numpy as np
import pytest
import torch  # noqa: F401  (before libgft.so is loaded: one HIP runtime)

import json_docs as J
import records as R
import schema_scale as S
from gofindthem_amd import _lib, group
from gofindthem_amd.finder import EmptyRgxEngine, Finder, GpuEngine
from json_docs import check_leaves, to_device

pytestmark = pytest.mark.gpu


def make_group(exprs, tags, rules, schema, include=None, exclude=None):
    f = Finder(GpuEngine(), EmptyRgxEngine(), False)
    for e, t in zip(exprs, tags):
        f.AddExpressionWithTag(e, t)
    g = group.NewFinderWithRules(f, rules)
    g.SetSchema(schema, include, exclude)
    return g


_PLAIN = {}


def plain_group(schema):
    """a group over S.SCHEMAS[schema] whose finder has one expression and no rules: for the calls that only decode.  Built once
    per module (the host compiles the 16 383 paths in seconds)"""
    if schema not in _PLAIN:
        _PLAIN[schema] = make_group(['"x"'], ["t"], {}, S.SCHEMAS[schema])
        check_leaves(_PLAIN[schema], ["{}"])                # (the engine exists from here on)
    return _PLAIN[schema]


@contextlib.contextmanager
def one_cu(g):
    """the engine of g on one CU: k_json runs 8 blocks, 32 waves.  No batch is in flight in this module."""
    L, e = _lib.load(), g.findthem.engine_handle()
    assert e and L.gft_set_cu_margin(e, S.ONE_CU) == 0
    try:
        yield
    finally:
        assert L.gft_set_cu_margin(e, 0) == 0


def statuses(ref):
    return [int(s) for s in ref[0]]


# ---- A. a wave walks document after document -----------------------------------------------------------------------------
def test_table_alignments_and_corpus_on_32_waves():
    g = plain_group("default")
    with one_cu(g):
        for case in (S.default_table(), S.alignments()):
            assert len(case.docs) > 2 * S.WAVES_ONE_CU
            assert statuses(check_leaves(g, case.docs)) == case.want
        case = S.corpus()
        ref = check_leaves(g, case.docs)
        assert all(ref[0][i] == 0 for i in range(len(case.docs)) if case.clean[i]) and 200 <= int((ref[0] != 0).sum()) and ref[5][0] > 2000


def test_default_grid_with_three_documents_per_wave():
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    case = S.tiled(n_cus)
    assert len(case.docs) >= 3 * 32 * n_cus + 37 and len(case.docs) > 2 * 32 * n_cus
    ref = check_leaves(plain_group("default"), case.docs)
    assert all(ref[0][i] == 0 for i in range(len(case.docs)) if case.clean[i]) and int((ref[0] != 0).sum()) >= 0.10 * len(case.docs)


def test_caps_on_32_waves():
    g, case = plain_group("default"), S.corpus()
    n_leaves, n_text = g.debug_json_leaves_ref(case.docs)[5]
    with one_cu(g):
        for caps in ((n_leaves - 1, n_text - 1), (3, n_text)):
            check_leaves(g, case.docs, caps)


def test_write_pass_skips_then_walks_on_32_waves():
    g, case = plain_group("default"), S.write_pass_order()
    with one_cu(g):
        ref = check_leaves(g, case.docs)
    assert ref[0][:64].all() and not ref[0][64:192].any() and ref[1][128] == 0 and ref[1][192] > 64


# ---- B. the walker at the size of a schema ----------------------------------------------------------------------------------
def test_trie_at_the_node_limit():
    g, case = plain_group("wide"), S.wide_cover()
    ref = check_leaves(g, case.docs)
    assert statuses(ref) == case.want and [int(f) for f in ref[2][:ref[5][0]]] == case.fields
    with one_cu(g):
        check_leaves(g, case.docs)


def test_visited_reset_strides_over_the_whole_bitset():
    g, case = plain_group("wide"), S.strided_reset()
    assert len(case.docs) >= 500
    with one_cu(g):
        ref = check_leaves(g, case.docs)
    assert statuses(ref) == [J.OK if c else J.DUP for c in case.clean]
    check_leaves(g, case.docs)


def test_nested_schema_of_3061_nodes():
    g, case = plain_group("nested"), S.nested()
    ref = check_leaves(g, case.docs)
    assert all(ref[0][i] == 0 for i in range(len(case.docs)) if case.clean[i]) and int((ref[0] != 0).sum()) >= 30 and ref[5][0] > 3000
    with one_cu(g):
        check_leaves(g, case.docs)


def test_keys_of_63_to_65535_bytes_and_their_near_misses():
    g, case = plain_group("long keys"), S.long_keys()
    ref = check_leaves(g, case.docs)
    assert statuses(ref) == case.want and [int(f) for f in ref[2][:ref[5][0]]] == case.fields
    with one_cu(g):
        check_leaves(g, case.docs)


def test_array_indices_of_up_to_four_digits():
    g, case = plain_group("indices"), S.indices()
    ref = check_leaves(g, case.docs)
    assert statuses(ref) == case.want and [int(f) for f in ref[2][:ref[5][0]]] == case.fields
    with one_cu(g):
        check_leaves(g, case.docs * 20)


# ---- C. the rule kernels at their limits -------------------------------------------------------------------------------------
def dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a).astype(dt)).cuda()


def rule_group(case):
    return make_group(case.exprs, case.tags, case.rules, case.schema, case.include, case.exclude)


def check_rules(case, g=None):
    """k_leaf_tags and k_record_rules over the case's leaf bitmap, clean and with garbage above the last expression == the oracle"""
    g = g or rule_group(case)
    assert g.rule_exprs() == case.exp.numbering
    for hits in (case.hits, case.dirty_hits()):
        got = g.debug_eval_rules_device(dev(hits.view(np.int32), np.int32), len(case.exprs), dev(case.field, np.int32), dev(case.rec_off, np.int64))
        assert np.array_equal(got.cpu().numpy().astype(np.uint32), case.want)
    return g


@pytest.mark.parametrize("name", S.RULE_CASES)
def test_rule_case(name):
    check_rules(S.RULE_CASES[name]())


def test_a_field_index_at_the_schema_size_is_refused_and_the_handle_still_answers():
    case = S.field_words_case()
    g = check_rules(case)
    field = case.field.copy()
    field[len(field) // 2] = 65535
    with pytest.raises(group.GroupFinderError) as ei:
        g.debug_eval_rules_device(dev(case.hits.view(np.int32), np.int32), len(case.exprs), dev(field, np.int32), dev(case.rec_off, np.int64))
    assert ei.value.code == _lib.GFT_E_INVALID
    check_rules(case, g)


# ---- D. end to end ---------------------------------------------------------------------------------------------------------
def test_nested_schema_end_to_end():
    exprs, tags, rules, docs, broken, clean = S.end_to_end()
    g = make_group(exprs, tags, rules, S.NESTED)
    records = [R.flatten(json.loads(d.decode("utf-8"))) for d in docs]
    blob, off, field, rec_off = g.pack_records(records)
    want = g.ProcessRecordsDevice(dev(blob, np.uint8), dev(off, np.int64), dev(field, np.int32), dev(rec_off, np.int64)).cpu().numpy()
    assert 30 < int(want.any(axis=1).sum()) and len(np.unique(want, axis=0)) > 10
    by_host = g.ProcessJsons(broken)
    assert sum(1 for r in by_host if r.get("rules")) > 30 and any("error" in r for r in by_host)
    for margin in (False, True):
        with one_cu(g) if margin else contextlib.nullcontext():
            rows, status = g.ProcessJsonsDevice(*to_device(docs))
            assert not status.cpu().numpy().any() and np.array_equal(rows.cpu().numpy(), want)
            assert g.ProcessJsonsSchema(broken) == by_host
            assert g.json_last()[0] >= sum(clean) and sum(g.json_last()) == len(broken)
