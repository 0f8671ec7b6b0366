"""The tag result document, host half: gft_debug_tags_json (csrc/tags_json.cpp -- the slot and field tables and the contract of the
tag document kernels in plain loops) against the restatement of tests/tags_json.py, and json.loads of it against
oracle/group_ref.py's tag_object.  Nothing here needs a GPU.

Every generated batch asserts that it is not vacuous (tags_json.assert_not_vacuous); the shapes that cannot hold one of the
properties -- one expression, one tag, one field, no tag of more than 32 slots, nothing excluded -- say so."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import records as R
import tag_entries as TE
import tags_json as TJ
from gofindthem_amd import _lib, group

_cases = {}


def case(key, make):
    if key not in _cases:
        _cases[key] = make()
    return _cases[key]


def case_E(E, n_records=40):
    return case(("E", E, n_records), lambda: TJ.Case(TJ.layout_exprs(TJ.sizes_for_E(E), E, nasty=E >= 64), TJ.make_schema(12), n_records, 1))


# ---- 0. the C ABI ----------------------------------------------------------------------------------------------------------------
def test_symbols_of_the_tag_document_calls_are_exported_and_declared():
    L = _lib.load()
    hdr = open(os.path.join(os.path.dirname(_lib.HERE), "include", "gft.h")).read()
    for name in ("gft_group_tags_json_device", "gft_debug_tags_json"):
        assert hasattr(L, name) and name in _lib.SYMBOLS and ("int %s(" % name) in hdr
    assert "#define GFT_TAGS_JSON_MAX_LEAVES %d" % TJ.MAX_LEAVES in hdr and TJ.MAX_LEAVES >= 256
    for name in ("TagsJsonDevice", "debug_tags_json"):
        assert hasattr(group.GroupFinder, name)


# ---- 1. expressions, slots and tags ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [1, 31, 32, 33, 64, 65, 1000])
def test_expression_counts_at_the_word_borders(E):
    c = case_E(E)
    assert c.E == E and c.g.findthem.n_expressions == E
    big = E >= 64                                                              # (a tag of 33 slots needs 34 expressions and the repeat)
    st = TJ.assert_not_vacuous(c.stats(), tags=E > 2, exprs=E > 2, shared=E > 1, second_word=big, fields=True)
    assert st["garbage"] > 0 or E % 32 == 0                                    # bits at and above E, ignored
    c.check()


@pytest.mark.parametrize("sizes", [[1, 2, 32, 33, 70], [70, 33, 32, 2, 1], [33], [32, 1], [2, 70]])
def test_tags_of_1_2_32_33_and_70_slots(sizes):
    exprs = TJ.layout_exprs(sizes, nasty=True)
    c = case(("slots", tuple(sizes)), lambda: TJ.Case(exprs, TJ.make_schema(9), 30, 2, density=0.1))
    per_tag = {}
    for (t, e), (ti, si) in TJ.slot_table(exprs).items():
        per_tag[t] = max(per_tag.get(t, 0), si + 1)
    assert sorted(per_tag.values()) == sorted(sizes) and b"" in per_tag
    TJ.assert_not_vacuous(c.stats(), tags=len(sizes) > 1, second_word=max(sizes) > 32)
    c.check()


@pytest.mark.parametrize("T", [1, 2, 33, 70])
def test_1_2_33_and_70_tags(T):
    sizes = [3] + [1 + (k % 3) for k in range(1, T)]
    c = case(("tags", T), lambda: TJ.Case(TJ.layout_exprs(sizes, nasty=True), TJ.make_schema(9), 30, 3, density=0.2))
    assert len({t for _, t in c.exprs}) == T and b"" in {t for _, t in c.exprs}
    TJ.assert_not_vacuous(c.stats(), tags=T > 1, second_word=False)            # (no tag of more than 32 slots)
    c.check()


def test_the_same_string_collapses_under_one_tag_and_gives_two_slots_under_two():
    exprs = [(b'"b"', b"t"), (b'"a"', b"t"), (b'"b"', b"t"), (b'"b"', b"u"), (b'"a" and "b"', b"t")]     # (descending, a repeat, a prefix)
    g = TJ.group_of(exprs, [b"f"])
    hits = np.asarray([[0b00101], [0b01111], [0b10010]], dtype=np.uint32)
    text, _, total = g.debug_tags_json(hits, 5, [0, 0, 0], [0, 1, 2, 3])
    assert bytes(text[:total]) == (b'[{"tags":{"t":{"f":["\\"b\\""]}}},{"tags":{"t":{"f":["\\"a\\"","\\"b\\""]},"u":{"f":["\\"b\\""]}}},'
                                   b'{"tags":{"t":{"f":["\\"a\\"","\\"a\\" and \\"b\\""]}}}]')


def test_the_order_is_unsigned_bytes():
    exprs = [(b'"\xc3\xa9"', b"\xff"), (b'"z"', b"\xff"), (b'"z"', b"z")]
    g = TJ.group_of(exprs, [b"\xc3", b"z"])
    text, _, total = g.debug_tags_json(np.asarray([[7], [7]], dtype=np.uint32), 3, [0, 1], [0, 2])
    assert bytes(text[:total]) == (b'[{"tags":{"z":{"z":["\\"z\\""],"\xc3":["\\"z\\""]},'
                                   b'"\xff":{"z":["\\"z\\"","\\"\xc3\xa9\\""],"\xc3":["\\"z\\"","\\"\xc3\xa9\\""]}}}]')


def test_tags_paths_and_expressions_with_quotes_backslashes_control_bytes_and_invalid_utf8():
    c = case("nasty", lambda: TJ.Case(TJ.layout_exprs([8, 7, 7], nasty=True), TJ.make_schema(14, nasty=True), 30, 4, density=0.3))
    blob = b"".join(e + t for e, t in c.exprs) + b"".join(c.schema)
    for needle in (b'"', b"\\", b"\x01", b"\x1f", b"\n", b"\r", b"\t", b"\x7f", b"\xff", "é".encode("utf-8")):
        assert needle in blob
    TJ.assert_not_vacuous(c.stats(), second_word=False)
    want = c.check()
    for piece in (b"\\u0001", b"\\u001f", b"\\n", b"\xff", b"\x7f", b'p\\"q', b"p\\\\b"):
        assert piece in want[0]


def test_fragment_lengths_from_4_bytes_to_5000():
    exprs = TJ.layout_exprs([12, 10, 10], lengths=True) + [(b'"y"', b"s")]
    c = case("lengths", lambda: TJ.Case(exprs, TJ.make_schema(18, lengths=True), 24, 5, exclude=None, density=0.3))
    frags = {len(TJ.escape(t)) + 2 for _, t in exprs} | {len(TJ.escape(e)) for e, _ in exprs} | {len(TJ.escape(p)) + 2 for p in c.schema}
    assert set(TJ.FRAGMENT_LENGTHS) <= frags
    TJ.assert_not_vacuous(c.stats(), second_word=False, masked=False)
    c.check()


# ---- 2. schemas -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reverse", [True, False])
@pytest.mark.parametrize("F", [1, 2, 33, 65])
def test_field_counts_and_schemas_in_reverse_byte_order(F, reverse):
    c = case(("F", F, reverse), lambda: TJ.Case(TJ.layout_exprs([33, 2], 40), TJ.make_schema(F, reverse), 30, 6))
    TJ.assert_not_vacuous(c.stats(), fields=F > 1, masked=F > 5)               # (the excluded subtree "x" is the sixth path)
    c.check()


def test_rank_is_byte_order_of_the_path_not_schema_order():
    exprs = [(b'"k"', b"t")]
    schema = [b"a0", b"items.index(2)", b"a.b", b"items.index(10)", b"a"]
    g = TJ.group_of(exprs, schema)
    hits = np.ones((5, 1), dtype=np.uint32)
    text, _, total = g.debug_tags_json(hits, 1, [0, 1, 2, 3, 4], [0, 5])
    got = bytes(text[:total])
    order = [got.index(TJ.escape(p) + b":[") for p in (b"a", b"a.b", b"a0", b"items.index(10)", b"items.index(2)")]
    assert order == sorted(order)


def test_a_tag_whose_only_hits_are_in_excluded_fields_is_absent():
    g = TJ.group_of([(b'"k"', b"t"), (b'"m"', b"u")], [b"ok", b"x"], None, ["x"])
    text, _, total = g.debug_tags_json(np.asarray([[1], [3]], dtype=np.uint32), 2, [0, 1], [0, 2])
    assert bytes(text[:total]) == b'[{"tags":{"t":{"ok":["\\"k\\""]}}}]'


# ---- 3. records -------------------------------------------------------------------------------------------------------------------
LEAF_COUNTS = [0, 1, 2, 63, 64, 65, 255, 256, 257, TJ.MAX_LEAVES - 1, TJ.MAX_LEAVES]


def wide_case(extra=()):
    leaves = LEAF_COUNTS + list(extra) + [3, 0, 5]
    return TJ.Case(TJ.layout_exprs([33, 2, 1], 40), TJ.make_schema(TJ.MAX_LEAVES + 40), len(leaves), 7, leaves=leaves, density=0.05)


def test_records_of_0_to_cap_leaves():
    c = case("wide", wide_case)
    assert [int(x) for x in np.diff(c.rec_off.astype(np.int64))][5:5 + 6] == LEAF_COUNTS[5:]   # (the first five are the planted ones)
    TJ.assert_not_vacuous(c.stats())
    c.check()


def test_a_record_of_cap_plus_1_leaves_is_refused_and_accepted_as_a_hole():
    c = case("too wide", lambda: wide_case([TJ.MAX_LEAVES + 1]))
    d = len(LEAF_COUNTS)
    assert int(c.rec_off[d + 1] - c.rec_off[d]) == TJ.MAX_LEAVES + 1
    with pytest.raises(group.GroupFinderError) as ei:
        c.host()
    assert ei.value.code == _lib.GFT_E_UNSUPPORTED and "GFT_TAGS_JSON_MAX_LEAVES" in str(ei.value)
    holes = np.zeros(len(c.rec_off) - 1, dtype=np.uint64)
    holes[d] = 77
    c.check(holes)


def test_a_field_named_twice_is_refused_and_the_handle_answers_afterwards():
    c = case_E(65)
    field = c.field.copy()
    d = next(d for d in range(len(c.rec_off) - 1) if c.rec_off[d + 1] - c.rec_off[d] >= 2 and c.valid[c.field[int(c.rec_off[d])]])
    field[int(c.rec_off[d]) + 1] = field[int(c.rec_off[d])]
    with pytest.raises(group.GroupFinderError) as ei:
        c.g.debug_tags_json(c.hits, c.E, field, c.rec_off)
    assert ei.value.code == _lib.GFT_E_UNSUPPORTED and "twice" in str(ei.value)
    bad = c.field.copy()
    bad[0] = len(c.schema)                                                     # what tag_entries_host's callers refuse, too
    with pytest.raises(group.GroupFinderError) as ei:
        c.g.debug_tags_json(c.hits, c.E, bad, c.rec_off)
    assert ei.value.code == _lib.GFT_E_INVALID
    c.check()


@pytest.mark.parametrize("n_records", [0, 1, 2, 63, 64, 65, 129])
def test_record_counts(n_records):
    c = case_E(65, n_records)
    if n_records >= 63:
        TJ.assert_not_vacuous(c.stats())
    want = c.check()
    if n_records == 0:
        assert want[0] == b"[]" and list(want[1]) == [1]


def test_a_finder_without_expressions():
    g = TJ.group_of([], [b"a", b"b"])
    text, out_off, total = g.debug_tags_json(np.zeros((3, 0), dtype=np.uint32), 0, [0, 1, 0], [0, 2, 2, 3])
    assert bytes(text[:total]) == b"[" + b",".join([TJ.EMPTY_DOC] * 3) + b"]" and list(out_off) == [1, 13, 25, 37]


def test_expressions_added_later_rebuild_the_table():
    g = TJ.group_of([(b'"b"', b"t")], [b"f"])
    text, _, total = g.debug_tags_json(np.asarray([[1]], dtype=np.uint32), 1, [0], [0, 1])
    assert bytes(text[:total]) == b'[{"tags":{"t":{"f":["\\"b\\""]}}}]'
    g.findthem.AddExpressionWithTag(b'"a"', b"t")
    text, _, total = g.debug_tags_json(np.asarray([[3]], dtype=np.uint32), 2, [0], [0, 1])
    assert bytes(text[:total]) == b'[{"tags":{"t":{"f":["\\"a\\"","\\"b\\""]}}}]'


# ---- 4. holes and caps -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["some", "all"])
@pytest.mark.parametrize("n_records", [1, 2, 40])
def test_holes_first_last_adjacent_and_everywhere(n_records, where):
    c = case_E(65, n_records)
    holes = TJ.make_holes(n_records, np.random.default_rng(n_records), where)
    if n_records == 40 and where == "some":
        assert holes[0] and holes[-1] and holes[20] and holes[21] and not holes[1]
        st = c.stats(holes)
        assert st["holes"] == 4 and st["two_tags"] > 0 and st["masked"] > 0
    want = c.check(holes)
    if where == "all":
        assert set(want[0]) <= {TJ.GUARD, ord("["), ord(","), ord("]")}        # separators, and not one byte of a document


@pytest.mark.parametrize("with_holes", [False, True])
def test_the_seven_caps(with_holes):
    c = case_E(65)
    holes = TJ.make_holes(40, np.random.default_rng(5)) if with_holes else None
    want = c.want(holes)
    caps = TJ.caps_for(want[0])
    assert len(set(caps)) == 7 and 0 < caps[-1] - (want[0].find(b'":["') + 3) < 7   # (the last one: inside an expression fragment)
    for cap in caps:
        TJ.assert_text(c.host(holes, cap), want, cap)


def test_count_only_and_a_refused_hole():
    c = case_E(65)
    n = len(c.rec_off) - 1
    out_off, total = np.zeros(n + 1, dtype=np.uint64), C.c_uint64(0)
    want = c.want()
    rc = c.g._L.gft_debug_tags_json(c.g._h, c.hits.ctypes.data, c.E, c.field.ctypes.data, c.rec_off.ctypes.data, n, len(c.field), None, None, 0,
                                    out_off.ctypes.data, C.byref(total))
    assert rc == 0 and total.value == len(want[0]) and np.array_equal(out_off, want[1])
    holes = np.zeros(n, dtype=np.uint64)
    holes[3] = 1 << 32
    with pytest.raises(group.GroupFinderError) as ei:
        c.host(holes)
    assert ei.value.code == _lib.GFT_E_INVALID
    c.check()                                                                  # the handle goes on answering


# ---- 5. against the oracle --------------------------------------------------------------------------------------------------------
def test_the_text_is_json_and_says_what_tag_object_says():
    """records of tests/records.py's generators, the leaf bitmap from the CPU oracle's ProcessText per leaf, the expectation
    oracle/group_ref.py's tag_object over the same records (tag_entries.tag_maps)"""
    rng = np.random.default_rng(9)
    schema = R.make_schema(12)
    exprs, tags = R.make_expressions(40, 7, rng)
    include, exclude = None, [schema[-1]]
    exp = R.Expectation(exprs, tags, {}, schema, include, exclude)
    valid = TE.valid_fields(schema, include, exclude)
    recs = [list(dict(rec).items()) for rec in TE.planted_records(40, schema, rng, valid)]     # (a field once per record)
    texts, field, rec_off = R.csr(recs, schema)
    hits = exp.hit_bitmap(texts)
    g = TJ.group_of([(e.encode(), t.encode()) for e, t in zip(exprs, tags)], [p.encode() for p in schema], include, exclude)
    text, _, total = g.debug_tags_json(hits, 40, field, rec_off)
    want = TE.tag_maps(exp, recs, hits)
    assert sum(len(m) for m in want) > 0 and any(len(m) >= 2 for m in want)
    assert json.loads(bytes(text[:total]).decode("utf-8")) == [{"tags": m} for m in want]
