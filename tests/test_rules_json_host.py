"""The rule result document, host half: gft_debug_rules_json (csrc/rules_json.cpp -- the fragment table and the contract of the
result kernels in plain loops) against the restatement of tests/rules_json.py, against json.loads, and byte for byte against the
document of gft_group_process_jsons.  Nothing here needs a GPU.

Every generated batch asserts that it is not vacuous (rules_json.assert_not_vacuous); the shapes that cannot hold one of the
properties -- a single rule, rules inside one word -- say so.  Fragments of 2 and 3 bytes cannot come out of AddRule (the shortest
expression is a quoted one-byte tag, 7 bytes escaped; the shortest name fragment is '"":[', 4 bytes): the stand-alone
tools/rules_json_check.cpp covers them through make_rule_fragments."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import records as R
import rules_json as RJ
from gofindthem_amd import _lib, group
from gofindthem_amd.engine import pack
from gofindthem_amd.finder import Finder

SIZES = {1: [1], 31: [20, 11], 32: [20, 11, 1], 33: [20, 13], 64: [20, 11, 33], 65: [20, 11, 1, 33]}


def sizes_of(R_, rng):
    return SIZES[R_] if R_ in SIZES else [20, 70] + RJ.sizes_for(R_ - 90, rng)


class Case:
    """one rule set with its group, its expressions as bytes and a batch of rows, made once and left unchanged"""

    def __init__(self, rules, n_docs, seed, density=0.1):
        self.g = RJ.group_of(rules)
        self.exprs = RJ.raw_rule_exprs(self.g)
        assert self.exprs == [(n, e) for n, es in rules for e in es]           # the bit order is the order the rules were laid out in
        self.rows = RJ.make_rows(self.exprs, n_docs, np.random.default_rng([seed, len(self.exprs), n_docs]), density)

    def check(self, hole_len=None, cap=None):
        want = RJ.expected(self.exprs, self.rows, hole_len)
        RJ.assert_text(self.g.debug_rules_json(self.rows, hole_len, cap), want, cap)
        return want


_cases = {}


def case_R(R_, n_docs=40):
    if (R_, n_docs) not in _cases:
        rng = np.random.default_rng([7, R_])
        _cases[(R_, n_docs)] = Case(RJ.layout_rules(sizes_of(R_, rng), nasty=True, lengths=R_ >= 64), n_docs, 1, 0.1 if R_ < 1000 else 0.01)
    return _cases[(R_, n_docs)]


# ---- 0. the C ABI ----------------------------------------------------------------------------------------------------------------
def test_symbols_of_the_result_calls_are_exported_and_declared():
    L = _lib.load()
    hdr = open(os.path.join(os.path.dirname(_lib.HERE), "include", "gft.h")).read()
    for name in ("gft_group_rules_json_device", "gft_debug_rules_json"):
        assert hasattr(L, name) and name in _lib.SYMBOLS and ("int %s(" % name) in hdr


# ---- 1. word borders of the rows, rules of every size at every place -----------------------------------------------------------
@pytest.mark.parametrize("R_", [1, 31, 32, 33, 64, 65, 2049, 4097])
def test_expression_counts_at_the_word_borders(R_):
    c = case_R(R_)
    # (R = 1: one rule of one expression; R <= 32: every rule inside the one word)
    s = RJ.assert_not_vacuous(c.exprs, c.rows, rules=R_ > 1, straddle=R_ > 32)
    assert s["garbage"] > 0 or R_ % 32 == 0                                    # bits above R in the last word, ignored
    c.check()


@pytest.mark.parametrize("begin", [0, 20, 31, 32])
@pytest.mark.parametrize("size", [1, 2, 33, 70])
def test_rules_of_1_2_33_and_70_expressions_beginning_at_bits_0_20_31_and_32(size, begin):
    sizes = RJ.sizes_with(size, begin)
    c = Case(RJ.layout_rules(sizes, nasty=True, lengths=True), 24, 2)
    assert RJ.rule_start(c.exprs, begin) == begin and (begin == 0 or RJ.rule_start(c.exprs, begin - 1) != begin)
    assert begin + size == len(c.exprs) or RJ.rule_start(c.exprs, begin + size) == begin + size
    # rows of this rule alone: its first bit, its last bit, all of it
    RW = c.rows.shape[1]
    for k, bits in enumerate(([begin], [begin + size - 1], list(range(begin, begin + size)))):
        c.rows[10 + k] = 0
        for i in bits:
            c.rows[10 + k, i // 32] |= np.uint32(1 << (i % 32))
    assert RW >= 2
    RJ.assert_not_vacuous(c.exprs, c.rows)
    c.check()


def test_fragment_lengths_from_4_bytes_to_5000():
    rules = RJ.short_fragment_rules() + RJ.layout_rules([3, 1, 33, 2, 5, 1, 1, 2, 4], lengths=True)
    c = Case(rules, 30, 3, density=0.3)
    frags = {len(RJ.escape(n)) + 2 for n, _ in c.exprs} | {len(RJ.escape(e)) for _, e in c.exprs}
    assert set(RJ.FRAGMENT_LENGTHS) <= frags
    RJ.assert_not_vacuous(c.exprs, c.rows)
    c.check()


def test_names_and_expressions_with_quotes_backslashes_control_bytes_and_invalid_utf8():
    c = Case(RJ.layout_rules([2] * 14, nasty=True), 20, 4, density=0.4)
    blob = b"".join(n + e for n, e in c.exprs)
    for needle in (b'"', b"\\", b"\x01", b"\x1f", b"\n", b"\r", b"\t", b"\x7f", b"\xff", "é".encode("utf-8")):
        assert needle in blob
    RJ.assert_not_vacuous(c.exprs, c.rows, straddle=False)                     # (28 expressions: one word)
    want = c.check()
    assert b"\\u0001" in want[0] and b"\\u001f" in want[0] and b"\\n" in want[0] and b"\xff" in want[0] and b"\x7f" in want[0]


# ---- 2. shapes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_docs", [0, 1, 2, 63, 64, 65, 129])
def test_document_counts(n_docs):
    c = case_R(65, n_docs)
    if n_docs >= 63:
        RJ.assert_not_vacuous(c.exprs, c.rows)
    want = c.check()
    if n_docs == 0:
        assert want[0] == b"[]" and list(want[1]) == [1]


def test_empty_rows_all_ones_rows_and_garbage_above_R():
    c = case_R(33, 12)
    rows = c.rows.copy()
    rows[0::3] = 0
    rows[1::3] = 0xFFFFFFFF                                                    # every bit of both words: 31 of them above R
    want = RJ.expected(c.exprs, rows)
    RJ.assert_text(c.g.debug_rules_json(rows), want)
    docs = want[0][1:-1].split(b'},{"rules"')
    assert len(docs) == 12 and want[0].count(RJ.EMPTY_DOC) >= 4


def test_a_group_without_rules():
    g = RJ.group_of([])
    rows = np.zeros((5, 0), dtype=np.uint32)
    text, out_off, total = g.debug_rules_json(rows)
    assert bytes(text[:total]) == b"[" + b",".join([RJ.EMPTY_DOC] * 5) + b"]"
    assert list(out_off) == [1 + 13 * k for k in range(6)]


def test_rules_added_later_rebuild_the_table():
    g = RJ.group_of([(b"a", [b'"x"'])])
    rows = np.asarray([[1]], dtype=np.uint32)
    text, _, total = g.debug_rules_json(rows)
    assert bytes(text[:total]) == b'[{"rules":{"a":["\\"x\\""]}}]'
    RJ.add_rule_raw(g, b"A", b'"y"')                                           # sorts in front: bit 0 is now A's
    text, _, total = g.debug_rules_json(np.asarray([[3]], dtype=np.uint32))
    assert bytes(text[:total]) == b'[{"rules":{"A":["\\"y\\""],"a":["\\"x\\""]}}]'


# ---- 3. holes and caps -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["some", "all"])
@pytest.mark.parametrize("n_docs", [1, 2, 40])
def test_holes_first_last_adjacent_and_everywhere(n_docs, where):
    c = case_R(65, n_docs)
    holes = RJ.make_holes(n_docs, np.random.default_rng(n_docs), where)
    if n_docs == 40 and where == "some":
        assert holes[0] and holes[-1] and holes[20] and holes[21] and not holes[1]
        RJ.assert_not_vacuous(c.exprs, c.rows[1:], holes[1:], holes=True)      # (document 0, the planted empty row, is a hole here)
    want = c.check(holes)
    if where == "all":
        assert set(want[0]) <= {RJ.GUARD, ord("["), ord(","), ord("]")}        # separators, and not one byte of a document


@pytest.mark.parametrize("with_holes", [False, True])
def test_the_seven_caps(with_holes):
    c = case_R(65)
    holes = RJ.make_holes(40, np.random.default_rng(5)) if with_holes else None
    want = RJ.expected(c.exprs, c.rows, holes)
    total = len(want[0])
    caps = RJ.caps_for(c.exprs, c.rows if not with_holes else c.rows[1:], total)
    assert len(set(caps)) == 7 and caps[-1] not in (0, 1, 11, 12, total - 1, total)
    for cap in caps:
        RJ.assert_text(c.g.debug_rules_json(c.rows, holes, cap), want, cap)


def test_count_only_and_a_refused_hole():
    c = case_R(65)
    out_off, total = np.zeros(41, dtype=np.uint64), C.c_uint64(0)
    want = RJ.expected(c.exprs, c.rows)
    assert c.g._L.gft_debug_rules_json(c.g._h, c.rows.ctypes.data, 40, None, None, 0, out_off.ctypes.data, C.byref(total)) == 0
    assert total.value == len(want[0]) and np.array_equal(out_off, want[1])
    holes = np.zeros(40, dtype=np.uint64)
    holes[3] = 1 << 32
    with pytest.raises(group.GroupFinderError) as ei:
        c.g.debug_rules_json(c.rows, holes)
    assert ei.value.code == _lib.GFT_E_INVALID
    c.check()                                                                  # the handle goes on answering


# ---- 4. against json.loads and against the host route's document -------------------------------------------------------------
def test_the_text_is_json_and_says_what_rules_from_bitmap_says():
    sizes = [20, 11, 1, 33, 2, 70, 1]
    rules = [("rule%02d é" % k, ['"t%d" or not "u%d:F.%d"' % (x, x, k) for x in range(s)]) for k, s in enumerate(sizes)]
    g = group.NewFinderWithRules(Finder(None, None, False, allow_no_device=True), dict(rules))
    exprs = RJ.raw_rule_exprs(g)
    rows = RJ.make_rows(exprs, 40, np.random.default_rng(6), 0.2)
    RJ.assert_not_vacuous(exprs, rows)
    text, _, total = g.debug_rules_json(rows)
    clean = rows.copy()
    clean[:, -1] &= np.uint32((1 << (len(exprs) % 32)) - 1)                    # (rules_from_bitmap takes every bit of a row for a rule's)
    assert len(exprs) % 32 and (clean != rows).any()
    assert json.loads(bytes(text[:total]).decode("utf-8")) == [{"rules": d} for d in g.rules_from_bitmap(clean)]


def host_route_text(g, raws):
    """the document of gft_group_process_jsons(..., what = 0), as bytes"""
    blob, off = pack(raws)
    need = C.c_uint64(0)
    rc = g._L.gft_group_process_jsons(g._h, blob.ctypes.data, off.ctypes.data, len(raws), None, 0, None, 0, 0, None, 0, C.byref(need))
    assert rc == _lib.GFT_E_INVALID and need.value > 0                         # (no buffer: the library keeps the document)
    buf = C.create_string_buffer(int(need.value))
    assert g._L.gft_group_last_result(g._h, C.cast(buf, C.c_void_p), int(need.value), C.byref(need)) == 0
    return buf.raw[:int(need.value) - 1]


def test_the_text_is_byte_for_byte_the_host_routes_document():
    """Documents made from records of the records.py generators, the rows from the oracle's rule evaluation of the same records.
    The host route scans and solves on the device, so on a box without one its documents with string leaves say "no HIP device";
    there the batch is one of documents without string leaves, whose rows are those of empty records -- the rules that a `not`
    makes true"""
    rng = np.random.default_rng(8)
    schema = [p for p in R.make_schema(24) if "." not in p]
    exprs, tags = R.make_expressions(12, 4, rng)
    rules = R.make_rules(14, 4, schema, rng)
    f = Finder(None, None, False, allow_no_device=True)
    for e, t in zip(exprs, tags):
        f.AddExpressionWithTag(e, t)
    g = group.NewFinderWithRules(f, rules)
    exp = R.Expectation(exprs, tags, rules, schema)
    assert [(n.decode(), e.decode()) for n, e in RJ.raw_rule_exprs(g)] == exp.numbering
    # (a field once per document; 60 records: the first 30 of this seed give three distinct rows, one short of what is asked below)
    recs = [list(dict(rec).items()) for rec in R.make_records(60, schema, rng)]
    raws = [json.dumps(dict(rec)).encode() for rec in recs]
    got = host_route_text(g, raws)
    on_device = b"no HIP device" not in got
    if not on_device:
        recs = [[] for _ in range(60)]
        raws = [json.dumps({schema[k % len(schema)]: k}).encode() for k in range(60)]
        got = host_route_text(g, raws)
    rows = exp.expected(recs)
    assert rows.any() and (not on_device or len({r.tobytes() for r in rows}) > 3)   # rules are true; with a device, rows differ
    text, _, total = g.debug_rules_json(rows)
    assert bytes(text[:total]) == got
