"""The rule result document on the device (csrc/gft_result.hip: result_count, result_scan, result_fill): RulesJsonDevice bit for bit
against the host contract gft_debug_rules_json and against the restatement of tests/rules_json.py -- text, out_off, total, the
guard bytes behind the cap and the bytes inside holes --, then gft_group_process_jsons_schema / _auto through the C ABI: their
bytes are those of a second group over the same finder created under GFT_DEVICE_RESULT=0, which serialises on the host.

Fragments of 2 and 3 bytes cannot come out of AddRule (tests/test_rules_json_host.py says why); the shortest here are 4 and 5."""
import ctypes as C
import json

import numpy as np
import pytest
import torch  # noqa: F401  (before libgft.so is loaded: one HIP runtime)

import json_docs as J
import records as R
import rules_json as RJ
import schema_scale as S
from gofindthem_amd import _lib, group
from gofindthem_amd.engine import pack
from gofindthem_amd.finder import EmptyRgxEngine, Finder, GpuEngine, PyRegexpEngine

pytestmark = pytest.mark.gpu


def dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a).astype(dt)).cuda()


_finder = None


def shared_finder():
    """one finder without expressions for every rule set of the kernel tests: each group installs its own fragment table on the
    finder's engine, as groups that share a finder do"""
    global _finder
    if _finder is None:
        _finder = Finder(GpuEngine(), EmptyRgxEngine(), False)
    return _finder


def sizes_to(R_, rng):
    sizes = []
    for s in (20, 13, 1, 33, 2, 70):                                           # (20 + 13: the second rule straddles bits 31 | 32)
        if sum(sizes) + s <= R_:
            sizes.append(s)
    return sizes + RJ.sizes_for(R_ - sum(sizes), rng)


class Case:
    """one rule set with its group on the shared finder, its expressions as bytes and a batch of rows, made once"""

    def __init__(self, sizes, n_docs, seed, density=0.1, rules=None):
        rules = RJ.layout_rules(sizes, nasty=True, lengths=True) if rules is None else rules
        self.g = RJ.group_of(rules, shared_finder())
        self.exprs = RJ.raw_rule_exprs(self.g)
        assert self.exprs == [(n, e) for n, es in rules for e in es]
        self.rows = RJ.make_rows(self.exprs, n_docs, np.random.default_rng([seed, len(self.exprs), n_docs]), density)

    def check(self, rows=None, holes=None, cap=None, restate=True):
        """the three launches == gft_debug_rules_json, every byte of both buffers (guard and hole bytes are 0xA5 on both sides),
        and == the restatement"""
        rows = self.rows if rows is None else rows
        ref = self.g.debug_rules_json(rows, holes, cap)
        got = self.g.RulesJsonDevice(dev(rows.view(np.int32), np.int32), None if holes is None else dev(holes, np.int64), cap)
        text, out_off = got[0].cpu().numpy(), got[1].cpu().numpy().astype(np.uint64)
        assert got[2] == ref[2]
        assert np.array_equal(out_off, ref[1])
        assert np.array_equal(text, ref[0])
        if restate:
            RJ.assert_text((text, out_off, got[2]), RJ.expected(self.exprs, rows, holes), cap)
        return ref


_cases = {}


def case_RW(RW, n_docs=40):
    if (RW, n_docs) not in _cases:
        R_ = RW * 32 - 5                                                       # (five bits of garbage room above R in the last word)
        _cases[(RW, n_docs)] = Case(sizes_to(R_, np.random.default_rng([9, RW])), n_docs, 1, 0.1 if RW < 32 else 0.01)
    return _cases[(RW, n_docs)]


# ---- 1. the three launches over seeded rows ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("RW", [1, 2, 3, 32, 33, 64, 65, 129])
def test_row_widths_on_both_sides_of_64_words(RW):
    c = case_RW(RW)
    assert c.rows.shape[1] == RW
    s = RJ.assert_not_vacuous(c.exprs, c.rows, straddle=RW > 1)                # (one word: no border to straddle)
    assert s["garbage"] > 0
    c.check()


@pytest.mark.parametrize("begin", [0, 20, 31, 32])
@pytest.mark.parametrize("size", [1, 2, 33, 70])
def test_rules_of_1_2_33_and_70_expressions_beginning_at_bits_0_20_31_and_32(size, begin):
    c = Case(RJ.sizes_with(size, begin), 24, 2)
    assert RJ.rule_start(c.exprs, begin) == begin and (begin == 0 or RJ.rule_start(c.exprs, begin - 1) != begin)
    for k, bits in enumerate(([begin], [begin + size - 1], list(range(begin, begin + size)))):
        c.rows[10 + k] = 0
        for i in bits:
            c.rows[10 + k, i // 32] |= np.uint32(1 << (i % 32))
    RJ.assert_not_vacuous(c.exprs, c.rows)
    c.check()


def test_fragment_lengths_from_4_bytes_to_5000():
    rules = RJ.short_fragment_rules() + RJ.layout_rules([3, 1, 33, 2, 5, 1, 1, 2, 4], lengths=True)
    c = Case(None, 30, 3, density=0.3, rules=rules)
    frags = {len(RJ.escape(n)) + 2 for n, _ in c.exprs} | {len(RJ.escape(e)) for _, e in c.exprs}
    assert set(RJ.FRAGMENT_LENGTHS) <= frags
    RJ.assert_not_vacuous(c.exprs, c.rows)
    c.check()


@pytest.mark.parametrize("n_docs", [0, 1, 63, 64, 65, 129])
def test_document_counts(n_docs):
    c = case_RW(3, n_docs)
    if n_docs >= 63:
        RJ.assert_not_vacuous(c.exprs, c.rows)
    ref = c.check()
    if n_docs == 0:
        assert bytes(ref[0][:2]) == b"[]" and ref[2] == 2
        c.check(cap=0)
        c.check(cap=1)


@pytest.mark.parametrize("RW", [3, 65])
@pytest.mark.parametrize("with_holes", [False, True])
def test_the_seven_caps(with_holes, RW):
    c = case_RW(RW)
    holes = RJ.make_holes(40, np.random.default_rng(5)) if with_holes else None
    total = len(RJ.expected(c.exprs, c.rows, holes)[0])
    caps = RJ.caps_for(c.exprs, c.rows if not with_holes else c.rows[1:], total)
    assert len(set(caps)) == 7
    for cap in caps:
        c.check(holes=holes, cap=cap)


@pytest.mark.parametrize("where", ["some", "all"])
@pytest.mark.parametrize("n_docs", [1, 2, 40])
def test_holes_first_last_adjacent_and_everywhere(n_docs, where):
    c = case_RW(3, n_docs)
    holes = RJ.make_holes(n_docs, np.random.default_rng(n_docs), where)
    rows = c.rows.copy()
    rows[holes != 0] = 0xFFFFFFFF                                              # a hole's row is not read: whatever it holds
    if n_docs == 40 and where == "some":
        assert holes[0] and holes[-1] and holes[20] and holes[21] and not holes[1]
        RJ.assert_not_vacuous(c.exprs, rows[1:], holes[1:], holes=True)
    ref = c.check(rows=rows, holes=holes)
    if where == "all":
        assert set(bytes(ref[0][:ref[2]])) <= {RJ.GUARD, ord("["), ord(","), ord("]")}


def one_cu_rows(c):
    """20 000 rows of three words: short documents, every 7th with a 5 000 byte fragment and two empty ones behind it"""
    long_bit = next(i for i, (n, e) in enumerate(c.exprs) if len(e) > 4000)
    rng = np.random.default_rng(11)
    short = RJ.make_rows(c.exprs, 200, rng, 0.05)
    short[:, long_bit // 32] &= np.uint32(~(1 << (long_bit % 32)) & 0xFFFFFFFF)
    rows = np.ascontiguousarray(short[rng.integers(7, 200, 20000)])           # (not the planted all-ones row)
    rows[:7] = short[:7]
    rows[8::7] = 0
    rows[9::7] = 0
    rows[7::7, long_bit // 32] |= np.uint32(1 << (long_bit % 32))
    return rows


def test_one_cu_waves_take_many_documents_long_ones_in_front_of_empty_ones():
    """the engine held to one CU: 8 blocks, 32 waves, 20 000 documents -- 625 trips a wave"""
    c = case_RW(3)
    rows = one_cu_rows(c)
    RJ.assert_not_vacuous(c.exprs, rows)
    L, e = _lib.load(), c.g.findthem.engine_handle()
    assert e and L.gft_set_cu_margin(e, S.ONE_CU) == 0
    try:
        ref = c.check(rows=rows)
    finally:
        assert L.gft_set_cu_margin(e, 0) == 0
    assert ref[2] > 20000 * 13 + 2800 * 5000


def test_profile_names_the_three_launches():
    c = case_RW(3)
    c.check(restate=False)
    L, e = _lib.load(), c.g.findthem.engine_handle()
    assert L.gft_profile_enable(e, 1) == 0
    try:
        c.g.RulesJsonDevice(dev(c.rows.view(np.int32), np.int32), None, 1 << 20)
        for name in (b"result_count", b"result_scan", b"result_fill"):
            ms, n = C.c_double(), C.c_uint64()
            assert L.gft_profile_read(e, name, C.byref(ms), C.byref(n)) == 0
            assert n.value == 1 and ms.value > 0
    finally:
        L.gft_profile_reset(e)
        L.gft_profile_enable(e, 0)


def test_refusals_leave_the_group_answering():
    c = case_RW(3)
    holes = np.zeros(40, dtype=np.uint64)
    holes[7] = 1 << 32
    with pytest.raises(group.GroupFinderError) as ei:
        c.g.RulesJsonDevice(dev(c.rows.view(np.int32), np.int32), dev(holes, np.int64))
    assert ei.value.code == _lib.GFT_E_INVALID and "hole" in str(ei.value)
    c.check(restate=False)
    # a handle over several devices
    f = Finder(GpuEngine(), EmptyRgxEngine(), False, devices=[0, 0])
    g = RJ.group_of(RJ.layout_rules([3, 2]), f)
    rows = np.asarray([[5], [0]], dtype=np.uint32)
    with pytest.raises(group.GroupFinderError) as ei:
        g.RulesJsonDevice(dev(rows.view(np.int32), np.int32))
    assert ei.value.code == _lib.GFT_E_UNSUPPORTED
    text, _, total = g.debug_rules_json(rows)
    assert json.loads(bytes(text[:total]).decode()) == [{"rules": d} for d in g.rules_from_bitmap(rows)]
    f.close()


# ---- 2. beside the record and tag calls; the existing JSON calls -------------------------------------------------------------------
def make_group(exprs, tags, schema=None, include=None, exclude=None, rules=None, regex=None, finder=None):
    if finder is None:
        finder = Finder(GpuEngine(), PyRegexpEngine() if regex else EmptyRgxEngine(), False)
        for e, t in zip(exprs, tags):
            finder.AddExpressionWithTag(e, t)
        if regex:
            finder.AddExpressionWithTag(*regex)
    g = group.NewFinderWithRules(finder, rules or {})
    if schema is not None:
        g.SetSchema(schema, include, exclude)
    return g


def group_pair(monkeypatch, *args, **kw):
    """a group that writes its result documents on the device and, over the same finder, one created under GFT_DEVICE_RESULT=0"""
    g_dev = make_group(*args, **kw)
    monkeypatch.setenv("GFT_DEVICE_RESULT", "0")
    g_host = make_group(*args, finder=g_dev.findthem, **kw)
    monkeypatch.delenv("GFT_DEVICE_RESULT")
    return g_dev, g_host


def c_document(g, raws, auto=None, cap=1 << 16):
    """gft_group_process_jsons_schema (auto None) or gft_group_process_jsons_auto (auto = (include, exclude)) through the C ABI ->
    (the document's bytes, whether it came through gft_group_last_result after a too-small buffer)"""
    raws = [r.encode("utf-8") if isinstance(r, str) else bytes(r) for r in raws]
    blob, off = pack(raws)
    need = C.c_uint64(0)
    buf = C.create_string_buffer(cap)
    head = (g._h, blob.ctypes.data, off.ctypes.data, len(raws))
    if auto is None:
        rc = g._L.gft_group_process_jsons_schema(*head, C.cast(buf, C.c_void_p), cap, C.byref(need))
    else:
        lists = []
        for lst in auto:
            j = json.dumps(list(lst)).encode() if lst else None
            lists += [j, len(j) if j else 0]
        rc = g._L.gft_group_process_jsons_auto(*head, *lists, C.cast(buf, C.c_void_p), cap, C.byref(need))
    again = rc == _lib.GFT_E_INVALID and need.value > cap
    if again:
        assert buf.raw[:8] == b"\0" * 8                                        # (nothing of the document in a buffer that cannot hold it)
        buf = C.create_string_buffer(int(need.value))
        rc = g._L.gft_group_last_result(g._h, C.cast(buf, C.c_void_p), int(need.value), C.byref(need))
    if rc != 0:
        raise g._err(rc)
    assert buf.raw[int(need.value) - 1] == 0
    return buf.raw[:int(need.value) - 1], again


def fills_of(g):
    ms, n = C.c_double(), C.c_uint64()
    rc = g._L.gft_profile_read(g.findthem.engine_handle(), b"result_fill", C.byref(ms), C.byref(n))
    return int(n.value) if rc == 0 else 0


def assert_same_documents(g_dev, g_host, raws, auto=None, want_again=None, device_route=None):
    """both groups, both answers byte for byte.  device_route (default: a batch with documents, a finder without regex terms): the
    device group ran result_fill exactly once; the group created under GFT_DEVICE_RESULT=0 never does"""
    L, e = g_dev._L, g_dev.findthem.engine_handle()
    if device_route is None:
        device_route = bool(raws) and not g_dev.findthem.GetRegexes()
    assert L.gft_profile_enable(e, 1) == 0
    try:
        L.gft_profile_reset(e)
        want, _ = c_document(g_host, raws, auto)
        assert fills_of(g_host) == 0
        L.gft_profile_reset(e)
        got, again = c_document(g_dev, raws, auto)
        assert fills_of(g_dev) == (1 if device_route else 0)
    finally:
        L.gft_profile_reset(e)
        L.gft_profile_enable(e, 0)
    assert got == want
    assert g_dev.json_last() == g_host.json_last()
    if want_again is not None:
        assert again is want_again
    return got


TABLE_EXPRS = ['"x"', '"y"', '"v"', '"lorem" and "ipsum"', '"p"', '"s" or "q"', '"first"', 'inord("lorem" and "ipsum")', '"é"', '"w"']
TABLE_TAGS = ["t0", "t1", "t0", "t2", "t1", "t2", "t0", "t3", "t3", "t1"]
TABLE_RULES = {"any x": ['"t0"', '"t0:a"', 'not "t1"'], 'quo"te': ['"t2" or "t3:m.n"', 'not "t0:k"'], "z\\last": ['"t1" and not "t2"']}


@pytest.mark.parametrize("schema", [J.SCHEMA, J.SCHEMA_UTF8, J.deep_schema(32), J.deep_schema(33)], ids=["default", "utf8", "deep32", "deep33"])
def test_process_jsons_schema_and_auto_on_the_table(schema, monkeypatch):
    """every document of tests/json_docs.py's table, every status: the documents the device hands back are holes that the host
    fills with their "rules" or their "error" """
    docs = [d for d in J.table() if d.schema == schema]
    exclude = [schema[3]] if len(schema) > 3 else None
    g_dev, g_host = group_pair(monkeypatch, TABLE_EXPRS, TABLE_TAGS, schema, None, exclude, TABLE_RULES)
    raws = [d.raw for d in docs]
    got = assert_same_documents(g_dev, g_host, raws)
    n_host = sum(d.status != 0 for d in docs)
    assert g_dev.json_last() == (len(docs) - n_host, n_host)
    parsed = json.loads(got.decode("utf-8", "replace"))
    assert parsed == g_dev.ProcessJsons(raws, None, exclude)
    if schema is J.SCHEMA:
        handed_back = [r for d, r in zip(docs, parsed) if d.status != 0]
        assert any(r.get("rules") for r in handed_back) and any("error" in r for r in handed_back)
        assert len({json.dumps(r) for d, r in zip(docs, parsed) if d.status == 0}) > 3
    auto = assert_same_documents(g_dev, g_host, raws, auto=(None, exclude))
    assert json.loads(auto.decode("utf-8", "replace")) == parsed
    assert c_document(g_dev, [])[0] == b"[]" and g_dev.json_last() == (0, 0)


def test_process_jsons_on_2000_generated_documents_and_a_too_small_buffer(monkeypatch):
    rng = np.random.default_rng(42)
    schema = R.make_schema(8)
    exprs, tags = R.make_expressions(40, 5, rng)
    rules = R.make_rules(40, 5, schema, rng)
    include, exclude = [schema[0], schema[1], schema[5]], [schema[1]]
    g_dev, g_host = group_pair(monkeypatch, exprs, tags, schema, include, exclude, rules)
    assert g_dev.rule_words() == 2
    docs = []
    for _ in range(2000):
        d = J.gen_doc(schema, rng, R.vocabulary())
        docs.append(J.mutate(d, rng) if rng.random() < 0.1 else d)
    # (the buffer of 64 KiB is too small: both answers come through gft_group_last_result, json_last keeps its meaning)
    got = assert_same_documents(g_dev, g_host, docs, want_again=True)
    n_device, n_host = g_dev.json_last()
    assert n_device + n_host == 2000 and n_device > 1700 and n_host > 0
    parsed = json.loads(got.decode("utf-8", "replace"))
    assert parsed == g_dev.ProcessJsons(docs, include, exclude)
    assert sum(1 for r in parsed if r.get("rules")) > 300 and any("error" in r for r in parsed)
    assert len({json.dumps(r, sort_keys=True) for r in parsed}) > 50          # the documents differ
    assert assert_same_documents(g_dev, g_host, docs, auto=(include, exclude), want_again=True) == got
    assert_same_documents(g_dev, g_host, docs[:10], want_again=False)           # (and a buffer that is large enough)


def test_every_document_a_hole_a_regex_finder_and_a_group_without_rules(monkeypatch):
    rng = np.random.default_rng(43)
    schema = R.make_schema(8)
    exprs, tags = R.make_expressions(40, 5, rng)
    rules = R.make_rules(12, 5, schema, rng)
    g_dev, g_host = group_pair(monkeypatch, exprs, tags, schema, None, None, rules)
    holes = [b"{", b'{"nosuch":"x"}', b'{"G0":"' + R.vocabulary()[0].encode() + b'","G0":"again"}', b"", b'{"G0.a":"dotted"}'] * 30
    got = assert_same_documents(g_dev, g_host, holes)
    assert g_dev.json_last() == (0, len(holes))
    parsed = json.loads(got.decode("utf-8", "replace"))
    assert any("error" in r for r in parsed) and any(r.get("rules") for r in parsed)
    # a regex finder: the whole batch on the host route, for both groups
    docs = [J.gen_doc(schema, rng, R.vocabulary()) for _ in range(100)]
    rx_dev, rx_host = group_pair(monkeypatch, exprs, tags, schema, None, None, rules, regex=(r'r"zq+x[0-9]"', "rxtag"))
    assert rx_dev.findthem.GetRegexes()
    assert c_document(rx_dev, docs)[0] == c_document(rx_host, docs)[0] == c_document(g_dev, docs)[0]
    assert rx_dev.json_last() == (0, 100) and g_dev.json_last()[0] > 80
    assert c_document(rx_dev, docs, auto=(None, None))[0] == c_document(g_dev, docs, auto=(None, None))[0]
    # a group without rules: every document the device decides is {"rules":{}}
    none_dev, none_host = group_pair(monkeypatch, exprs, tags, schema, None, None, {})
    got = assert_same_documents(none_dev, none_host, docs + [b"{"])
    parsed = json.loads(got.decode("utf-8", "replace"))
    assert parsed[:100] == [{"rules": {}}] * 100 and "error" in parsed[100]
    assert got.startswith(b"[" + b",".join([RJ.EMPTY_DOC] * 100) + b',{"error":')


def test_the_text_buffer_grows_beside_the_record_and_tag_calls(monkeypatch):
    """a small JSON batch, ProcessRecordsDevice and TagRecordsDevice, a larger JSON batch, the small one again, on one handle: the
    documents are those of the host serialisation, the rows and entries those of a handle that made no result call"""
    rng = np.random.default_rng(44)
    schema = R.make_schema(8)
    exprs, tags = R.make_expressions(40, 5, rng)
    rules = R.make_rules(40, 5, schema, rng)
    g_dev, g_host = group_pair(monkeypatch, exprs, tags, schema, None, None, rules)
    clean = make_group(exprs, tags, schema, None, None, rules)
    recs = R.make_records(500, schema, rng)

    def record_calls(g, result=True):
        blob, off, field, rec_off = g.pack_records(recs)
        args = (dev(blob, np.uint8), dev(off, np.int64), dev(field, np.int32), dev(rec_off, np.int64))
        rows = g.ProcessRecordsDevice(*args)
        ent = g.TagRecordsDevice(*args)
        text = g.RulesJsonDevice(rows) if result else None
        return rows.cpu().numpy(), [x.cpu().numpy() for x in ent[:3]], ent[4], text

    small = [J.gen_doc(schema, rng, R.vocabulary()) for _ in range(50)]
    large = [J.gen_doc(schema, rng, R.vocabulary()) for _ in range(3000)]
    want_rows, want_ent, want_total, _ = record_calls(clean, result=False)
    assert want_rows.any() and want_total > 0
    for docs in (small, large, small):
        assert c_document(g_dev, docs)[0] == c_document(g_host, docs)[0]
        rows, ent, total, text = record_calls(g_dev)
        assert np.array_equal(rows, want_rows) and total == want_total and all(np.array_equal(a, b) for a, b in zip(ent, want_ent))
        ref = g_dev.debug_rules_json(rows.view(np.uint32))
        assert text[2] == ref[2] and np.array_equal(text[0].cpu().numpy(), ref[0])
        parsed = json.loads(bytes(ref[0][:ref[2]]).decode())
        assert parsed == [{"rules": d} for d in g_dev.rules_from_bitmap(rows.view(np.uint32))]
