"""The tag result document on the device (csrc/gft_tagdoc.hip: tagdoc_slots, tagdoc_count, tagdoc_scan, tagdoc_fill):
TagsJsonDevice bit for bit against the host contract gft_debug_tags_json and against the restatement of tests/tags_json.py --
text, out_off, total, the guard bytes behind the cap and the bytes inside holes --, then gft_group_tag_jsons_schema / _auto
through the C ABI: their bytes are those of a second group over the same finder created under GFT_DEVICE_RESULT=0, which
serialises on the host."""
import ctypes as C
import json

import numpy as np
import pytest
import torch  # noqa: F401  (before libgft.so is loaded: one HIP runtime)

import json_docs as J
import records as R
import schema_scale as S
import tags_json as TJ
from gofindthem_amd import _lib, group
from gofindthem_amd.engine import pack
from gofindthem_amd.finder import EmptyRgxEngine, Finder, GpuEngine, PyRegexpEngine

pytestmark = pytest.mark.gpu


def dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a).astype(dt)).cuda()


def device_call(g, hits, field, rec_off, holes=None, cap=None):
    return g.TagsJsonDevice(dev(hits.view(np.int32), np.int32), dev(field, np.int32), dev(rec_off, np.int64),
                            None if holes is None else dev(holes, np.int64), cap)


def check(c, holes=None, cap=None, restate=True, hits=None, field=None, rec_off=None):
    """the four launches == gft_debug_tags_json, every byte of both buffers (guard and hole bytes are 0xA5 on both sides) and
    out_off, and == the restatement"""
    hits = c.hits if hits is None else hits
    field = c.field if field is None else field
    rec_off = c.rec_off if rec_off is None else rec_off
    ref = c.g.debug_tags_json(hits, c.E, field, rec_off, holes, cap)
    got = device_call(c.g, hits, field, rec_off, holes, cap)
    text, out_off = got[0].cpu().numpy(), got[1].cpu().numpy().astype(np.uint64)
    assert got[2] == ref[2]
    assert np.array_equal(out_off, ref[1])
    assert np.array_equal(text, ref[0])
    if restate:
        TJ.assert_text((text, out_off, got[2]), TJ.expected(c.exprs, c.schema, c.valid, hits, field, rec_off, holes), cap)
    return ref


_cases = {}


def case(key, make):
    if key not in _cases:
        _cases[key] = make()
    return _cases[key]


def case_E(E, n_records=40):
    return case(("E", E, n_records),
                lambda: TJ.Case(TJ.layout_exprs(TJ.sizes_for_E(E), E, nasty=E >= 64), TJ.make_schema(12), n_records, 1, device=True))


# ---- 1. the four launches over seeded batches ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [1, 31, 32, 33, 64, 65, 1000])
def test_expression_counts_at_the_word_borders(E):
    c = case_E(E)
    st = TJ.assert_not_vacuous(c.stats(), tags=E > 2, exprs=E > 2, shared=E > 1, second_word=E >= 64)
    assert st["garbage"] > 0 or E % 32 == 0
    check(c)


@pytest.mark.parametrize("sizes", [[1, 2, 32, 33, 70], [70, 33, 32, 2, 1], [33]])
def test_tags_of_1_2_32_33_and_70_slots(sizes):
    c = case(("slots", tuple(sizes)), lambda: TJ.Case(TJ.layout_exprs(sizes, nasty=True), TJ.make_schema(9), 30, 2, density=0.1, device=True))
    TJ.assert_not_vacuous(c.stats(), tags=len(sizes) > 1)
    check(c)


@pytest.mark.parametrize("T", [1, 2, 33, 70])
def test_1_2_33_and_70_tags(T):
    sizes = [3] + [1 + (k % 3) for k in range(1, T)]
    c = case(("tags", T), lambda: TJ.Case(TJ.layout_exprs(sizes, nasty=True), TJ.make_schema(9), 30, 3, density=0.2, device=True))
    TJ.assert_not_vacuous(c.stats(), tags=T > 1, second_word=False)
    check(c)


def test_nasty_bytes_and_fragment_lengths_from_4_bytes_to_5000():
    c = case("nasty", lambda: TJ.Case(TJ.layout_exprs([8, 7, 7], nasty=True), TJ.make_schema(14, nasty=True), 30, 4, density=0.3, device=True))
    TJ.assert_not_vacuous(c.stats(), second_word=False)
    check(c)
    exprs = TJ.layout_exprs([12, 10, 10], lengths=True) + [(b'"y"', b"s")]
    c = case("lengths", lambda: TJ.Case(exprs, TJ.make_schema(18, lengths=True), 24, 5, exclude=None, density=0.3, device=True))
    frags = {len(TJ.escape(t)) + 2 for _, t in exprs} | {len(TJ.escape(e)) for e, _ in exprs} | {len(TJ.escape(p)) + 2 for p in c.schema}
    assert set(TJ.FRAGMENT_LENGTHS) <= frags
    TJ.assert_not_vacuous(c.stats(), second_word=False, masked=False)
    check(c)


@pytest.mark.parametrize("reverse", [True, False])
@pytest.mark.parametrize("F", [1, 2, 33, 65])
def test_field_counts_and_schemas_in_reverse_byte_order(F, reverse):
    c = case(("F", F, reverse), lambda: TJ.Case(TJ.layout_exprs([33, 2], 40), TJ.make_schema(F, reverse), 30, 6, device=True))
    TJ.assert_not_vacuous(c.stats(), fields=F > 1, masked=F > 5)
    check(c)


LEAF_COUNTS = [0, 1, 2, 63, 64, 65, 255, 256, 257, TJ.MAX_LEAVES - 1, TJ.MAX_LEAVES]


def wide_case():
    leaves = LEAF_COUNTS + [TJ.MAX_LEAVES + 1, 3, 0, 5]
    return TJ.Case(TJ.layout_exprs([33, 2, 1], 40), TJ.make_schema(TJ.MAX_LEAVES + 40), len(leaves), 7, leaves=leaves, density=0.05, device=True)


def test_records_of_0_to_cap_leaves_and_cap_plus_1_as_a_hole():
    c = case("wide", wide_case)
    d = len(LEAF_COUNTS)
    assert int(c.rec_off[d + 1] - c.rec_off[d]) == TJ.MAX_LEAVES + 1
    holes = np.zeros(len(c.rec_off) - 1, dtype=np.uint64)
    holes[d] = 77
    TJ.assert_not_vacuous(c.stats(holes), holes=True)
    check(c, holes=holes)


@pytest.mark.parametrize("n_records", [0, 1, 2, 63, 64, 65, 129])
def test_record_counts(n_records):
    c = case_E(65, n_records)
    if n_records >= 63:
        TJ.assert_not_vacuous(c.stats())
    ref = check(c)
    if n_records == 0:
        assert bytes(ref[0][:2]) == b"[]" and ref[2] == 2
        check(c, cap=0)
        check(c, cap=1)


@pytest.mark.parametrize("with_holes", [False, True])
def test_the_seven_caps(with_holes):
    c = case_E(65)
    holes = TJ.make_holes(40, np.random.default_rng(5)) if with_holes else None
    caps = TJ.caps_for(c.want(holes)[0])
    assert len(set(caps)) == 7
    for cap in caps:
        check(c, holes=holes, cap=cap)


@pytest.mark.parametrize("where", ["some", "all"])
@pytest.mark.parametrize("n_records", [1, 2, 40])
def test_holes_first_last_adjacent_and_everywhere(n_records, where):
    c = case_E(65, n_records)
    holes = TJ.make_holes(n_records, np.random.default_rng(n_records), where)
    ref = check(c, holes=holes)
    if where == "all":
        assert set(bytes(ref[0][:ref[2]])) <= {TJ.GUARD, ord("["), ord(","), ord("]")}


def test_one_cu_waves_take_many_records():
    """the engine held to one CU: 8 blocks, 32 waves, 20 000 records -- 625 trips a wave, the LDS arrays reused every trip"""
    c = case_E(65, 200)
    TJ.assert_not_vacuous(c.stats())
    reps = 100
    n_leaves = len(c.field)
    hits, field = np.tile(c.hits, (reps, 1)), np.tile(c.field, reps)
    rec_off = np.concatenate([[0], (c.rec_off[1:].astype(np.int64)[None, :] + n_leaves * np.arange(reps)[:, None]).reshape(-1)]).astype(np.uint64)
    assert len(rec_off) == 20001 and int(rec_off[-1]) == len(field)
    L, e = _lib.load(), c.g.findthem.engine_handle()
    assert e and L.gft_set_cu_margin(e, S.ONE_CU) == 0
    try:
        ref = check(c, restate=False, hits=hits, field=field, rec_off=rec_off)
    finally:
        assert L.gft_set_cu_margin(e, 0) == 0
    one = c.want()[0]
    assert bytes(ref[0][:ref[2]]) == b"[" + b",".join([one[1:-1]] * reps) + b"]"


def test_profile_names_the_four_launches():
    c = case_E(65)
    L, e = _lib.load(), c.g.findthem.engine_handle()
    assert L.gft_profile_enable(e, 1) == 0
    try:
        device_call(c.g, c.hits, c.field, c.rec_off, None, 1 << 20)
        for name in (b"tagdoc_slots", b"tagdoc_count", b"tagdoc_scan", b"tagdoc_fill"):
            ms, n = C.c_double(), C.c_uint64()
            assert L.gft_profile_read(e, name, C.byref(ms), C.byref(n)) == 0
            assert n.value == 1 and ms.value > 0
    finally:
        L.gft_profile_reset(e)
        L.gft_profile_enable(e, 0)


def test_refusals_leave_the_group_answering():
    c = case("wide", wide_case)
    n = len(c.rec_off) - 1

    def refused(code, word, **kw):
        with pytest.raises(group.GroupFinderError) as ei:
            device_call(c.g, kw.get("hits", c.hits), kw.get("field", c.field), kw.get("rec_off", c.rec_off), kw.get("holes"))
        assert ei.value.code == code and word in str(ei.value)
    wide_hole = np.zeros(n, dtype=np.uint64)
    wide_hole[len(LEAF_COUNTS)] = 50
    refused(_lib.GFT_E_UNSUPPORTED, "GFT_TAGS_JSON_MAX_LEAVES")               # the record of cap + 1 leaves, no hole
    holes = wide_hole.copy()
    holes[2] = 1 << 32
    refused(_lib.GFT_E_INVALID, "hole", holes=holes)
    twice = c.field.copy()
    d = LEAF_COUNTS.index(257)
    first = int(c.rec_off[d])
    a, b = [l for l in range(first, first + 257) if c.valid[c.field[l]]][:2]
    twice[b] = twice[a]
    refused(_lib.GFT_E_UNSUPPORTED, "twice", field=twice, holes=wide_hole)
    outside = c.field.copy()
    outside[first] = len(c.schema)
    refused(_lib.GFT_E_INVALID, "outside the schema", field=outside, holes=wide_hole)
    descends = c.rec_off.copy()
    descends[3], descends[4] = descends[4], descends[3]
    assert descends[3] > descends[4]
    refused(_lib.GFT_E_INVALID, "rec_off", rec_off=descends, holes=wide_hole)
    check(c, holes=wide_hole, restate=False)                                   # the handle goes on answering
    # a handle over several devices
    f = Finder(GpuEngine(), EmptyRgxEngine(), False, devices=[0, 0])
    f.AddExpressionWithTag('"k"', "t")
    g = group.NewFinderWithRules(f, {})
    g.SetSchema(["a"])
    with pytest.raises(group.GroupFinderError) as ei:
        device_call(g, np.ones((1, 1), dtype=np.uint32), np.zeros(1, dtype=np.uint32), np.asarray([0, 1], dtype=np.uint64))
    assert ei.value.code == _lib.GFT_E_UNSUPPORTED
    f.close()


# ---- 2. gft_group_tag_jsons_schema / _auto -----------------------------------------------------------------------------------------
def make_group(exprs, tags, schema=None, include=None, exclude=None, regex=None, finder=None):
    if finder is None:
        finder = Finder(GpuEngine(), PyRegexpEngine() if regex else EmptyRgxEngine(), False)
        for e, t in zip(exprs, tags):
            finder.AddExpressionWithTag(e, t)
        if regex:
            finder.AddExpressionWithTag(*regex)
    g = group.NewFinderWithRules(finder, {})
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
    """gft_group_tag_jsons_schema (auto None) or gft_group_tag_jsons_auto (auto = (include, exclude)) through the C ABI -> (the
    document's bytes, whether it came through gft_group_last_result after a too-small buffer)"""
    raws = [r.encode("utf-8") if isinstance(r, str) else bytes(r) for r in raws]
    blob, off = pack(raws)
    need = C.c_uint64(0)
    buf = C.create_string_buffer(cap)
    head = (g._h, blob.ctypes.data, off.ctypes.data, len(raws))
    if auto is None:
        rc = g._L.gft_group_tag_jsons_schema(*head, C.cast(buf, C.c_void_p), cap, C.byref(need))
    else:
        lists = []
        for lst in auto:
            j = json.dumps(list(lst)).encode() if lst else None
            lists += [j, len(j) if j else 0]
        rc = g._L.gft_group_tag_jsons_auto(*head, *lists, C.cast(buf, C.c_void_p), cap, C.byref(need))
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
    rc = g._L.gft_profile_read(g.findthem.engine_handle(), b"tagdoc_fill", C.byref(ms), C.byref(n))
    return int(n.value) if rc == 0 else 0


def assert_same_documents(g_dev, g_host, raws, auto=None, want_again=None, device_route=None):
    """both groups, both answers byte for byte and the same json_last.  device_route (default: a batch with documents, a finder
    without regex terms): the device group ran tagdoc_fill exactly once; the group created under GFT_DEVICE_RESULT=0 never does"""
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


TABLE_EXPRS = ['"x"', '"y"', '"v"', '"lorem" and "ipsum"', '"p"', '"s" or "q"', '"first"', 'inord("lorem" and "ipsum")', '"é"', '"w"', '"x"']
TABLE_TAGS = ["t0", "t1", "t0", "t2", "t1", "", "t0", "t3", "t3", "t1", "t0"]


@pytest.mark.parametrize("schema", [J.SCHEMA, J.SCHEMA_UTF8, J.deep_schema(32), J.deep_schema(33)], ids=["default", "utf8", "deep32", "deep33"])
def test_tag_jsons_schema_and_auto_on_the_table(schema, monkeypatch):
    """every document of tests/json_docs.py's table, every status: the documents the device hands back are holes that the host
    fills with their "tags" or their "error" """
    docs = [d for d in J.table() if d.schema == schema]
    exclude = [schema[3]] if len(schema) > 3 else None
    g_dev, g_host = group_pair(monkeypatch, TABLE_EXPRS, TABLE_TAGS, schema, None, exclude)
    raws = [d.raw for d in docs]
    got = assert_same_documents(g_dev, g_host, raws)
    n_host = sum(d.status != 0 for d in docs)
    assert g_dev.json_last() == (len(docs) - n_host, n_host)
    parsed = json.loads(got.decode("utf-8", "replace"))
    assert parsed == g_dev.TagJsons(raws, None, exclude)
    if schema is J.SCHEMA:
        handed_back = [r for d, r in zip(docs, parsed) if d.status != 0]
        assert any(r.get("tags") for r in handed_back) and any("error" in r for r in handed_back)
        assert len({json.dumps(r) for d, r in zip(docs, parsed) if d.status == 0}) > 3
    auto = assert_same_documents(g_dev, g_host, raws, auto=(None, exclude))
    assert json.loads(auto.decode("utf-8", "replace")) == parsed
    assert c_document(g_dev, [])[0] == b"[]" and g_dev.json_last() == (0, 0)


def test_tag_jsons_on_2000_generated_documents_and_a_too_small_buffer(monkeypatch):
    rng = np.random.default_rng(42)
    schema = R.make_schema(8)
    exprs, tags = R.make_expressions(40, 5, rng)
    include, exclude = [schema[0], schema[1], schema[5]], [schema[1]]
    g_dev, g_host = group_pair(monkeypatch, exprs, tags, schema, include, exclude)
    docs = []
    for _ in range(2000):
        d = J.gen_doc(schema, rng, R.vocabulary())
        docs.append(J.mutate(d, rng) if rng.random() < 0.1 else d)
    got = assert_same_documents(g_dev, g_host, docs, want_again=True)
    n_device, n_host = g_dev.json_last()
    assert n_device + n_host == 2000 and n_device > 1700 and n_host > 0
    parsed = json.loads(got.decode("utf-8", "replace"))
    assert parsed == g_dev.TagJsons(docs, include, exclude)
    assert sum(1 for r in parsed if r.get("tags")) > 300 and any("error" in r for r in parsed)
    assert any(len(r.get("tags", {})) >= 2 for r in parsed) and len({json.dumps(r, sort_keys=True) for r in parsed}) > 50
    assert assert_same_documents(g_dev, g_host, docs, auto=(include, exclude), want_again=True) == got
    assert_same_documents(g_dev, g_host, docs[:10], want_again=False)           # (and a buffer that is large enough)


def test_every_document_a_hole_a_regex_finder_and_a_finder_without_expressions(monkeypatch):
    rng = np.random.default_rng(43)
    schema = R.make_schema(8)
    exprs, tags = R.make_expressions(40, 5, rng)
    g_dev, g_host = group_pair(monkeypatch, exprs, tags, schema)
    every = " ".join(R.vocabulary()).encode()                                  # (a string that makes every expression true)
    holes = [b"{", b'{"nosuch":"x"}', b'{"G0":"' + every + b'","G0":"' + every + b'"}', b"", b'{"G0.a":"dotted"}'] * 30
    got = assert_same_documents(g_dev, g_host, holes)
    assert g_dev.json_last() == (0, len(holes))
    parsed = json.loads(got.decode("utf-8", "replace"))
    assert any("error" in r for r in parsed) and any(r.get("tags") for r in parsed)
    # a regex finder: the whole batch on the host route, for both groups
    docs = [J.gen_doc(schema, rng, R.vocabulary()) for _ in range(100)]
    rx_dev, rx_host = group_pair(monkeypatch, exprs, tags, schema, regex=(r'r"zq+x[0-9]"', "rxtag"))
    assert rx_dev.findthem.GetRegexes()
    assert assert_same_documents(rx_dev, rx_host, docs) == c_document(g_dev, docs)[0]
    assert rx_dev.json_last() == (0, 100) and g_dev.json_last()[0] > 80
    assert c_document(rx_dev, docs, auto=(None, None))[0] == c_document(g_dev, docs, auto=(None, None))[0]
    # a finder without expressions: every document the device decides is {"tags":{}}
    none_dev, none_host = group_pair(monkeypatch, [], [], schema)
    got = assert_same_documents(none_dev, none_host, docs + [b"{"])
    assert got.startswith(b"[" + b",".join([TJ.EMPTY_DOC] * 100) + b',{"error":')


def test_one_document_wider_than_the_cap_among_ordinary_ones(monkeypatch):
    F = TJ.MAX_LEAVES + 60
    schema = ["f%04d" % k for k in range(F)]
    exprs, tags = ['"lorem"', '"ipsum"', '"lorem" and "dolor"'], ["a", "b", "a"]
    g_dev, g_host = group_pair(monkeypatch, exprs, tags, schema, None, [schema[5]])
    words = ["lorem", "ipsum", "dolor sit lorem", "amet"]
    wide = json.dumps({schema[k]: words[k % 4] for k in range(F)})
    at_cap = json.dumps({schema[k]: words[k % 4] for k in range(TJ.MAX_LEAVES)})
    docs = [json.dumps({schema[k]: words[k % 4], schema[k + 7]: "ipsum lorem"}) for k in range(20)] + [wide, at_cap, "{", json.dumps({schema[3]: "dolor lorem"})]
    got = assert_same_documents(g_dev, g_host, docs)
    assert g_dev.json_last() == (len(docs) - 1, 1)                             # (the wide document was decided on the device)
    parsed = json.loads(got.decode())
    assert parsed == g_dev.TagJsons(docs, None, [schema[5]])
    assert len(parsed[20]["tags"]["a"]) > TJ.MAX_LEAVES // 2 and len(parsed[21]["tags"]["a"]) >= TJ.MAX_LEAVES // 2
    assert assert_same_documents(g_dev, g_host, docs, auto=(None, [schema[5]])) == got


def test_the_text_buffer_grows_beside_the_record_tag_and_rule_calls(monkeypatch):
    """a small JSON batch, ProcessRecordsDevice, TagRecordsDevice and ProcessJsonsSchema, a larger JSON batch, the small one again,
    on one handle: the documents are those of the host serialisation, the rows and entries those of a handle that made no tag
    document call"""
    rng = np.random.default_rng(44)
    schema = R.make_schema(8)
    exprs, tags = R.make_expressions(40, 5, rng)
    rules = R.make_rules(40, 5, schema, rng)
    g_dev, g_host = group_pair(monkeypatch, exprs, tags, schema)
    clean = make_group(exprs, tags, schema)
    for g in (g_dev, g_host, clean):
        g.AddRules(rules)
    recs = R.make_records(500, schema, rng)

    def other_calls(g, docs):
        blob, off, field, rec_off = g.pack_records(recs)
        args = (dev(blob, np.uint8), dev(off, np.int64), dev(field, np.int32), dev(rec_off, np.int64))
        rows = g.ProcessRecordsDevice(*args)
        ent = g.TagRecordsDevice(*args)
        return rows.cpu().numpy(), [x.cpu().numpy() for x in ent[:3]], ent[4], g.ProcessJsonsSchema(docs)

    small = [J.gen_doc(schema, rng, R.vocabulary()) for _ in range(50)]
    large = [J.gen_doc(schema, rng, R.vocabulary()) for _ in range(3000)]
    for docs in (small, large, small):
        want_rows, want_ent, want_total, want_rules = other_calls(clean, docs)
        assert want_rows.any() and want_total > 0
        assert c_document(g_dev, docs)[0] == c_document(g_host, docs)[0]
        rows, ent, total, rules_doc = other_calls(g_dev, docs)
        assert np.array_equal(rows, want_rows) and total == want_total and all(np.array_equal(a, b) for a, b in zip(ent, want_ent))
        assert rules_doc == want_rules
