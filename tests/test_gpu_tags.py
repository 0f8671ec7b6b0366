"""Tag entries on the GPU (csrc/gft_tags.hip): the three launches over leaf bitmaps of the CPU oracle, bit for bit against
gft_debug_tag_entries (which tests/test_tags_host.py holds against the restatement of tests/tag_entries.py); then the calls on
top -- TagRecordsDevice and both routes of TagRecords against the oracle's tag maps, TagJsonsDevice against TagRecordsDevice over
the flattened documents, TagJsonsSchema and TagJsonsAuto against TagJsons as Python objects.  The generated batches assert that
they are not vacuous (tag_entries.assert_not_vacuous)."""
import ctypes as C
import json

import numpy as np
import pytest
import torch  # noqa: F401  (before libgft.so is loaded: one HIP runtime)

import json_docs as J
import records as R
import schema_scale as S
import tag_entries as TE
from gofindthem_amd import _lib, group
from gofindthem_amd.finder import EmptyRgxEngine, Finder, GpuEngine, PyRegexpEngine
from json_docs import to_device
from tolower_cases import ref_lower

pytestmark = pytest.mark.gpu

GUARD_DEV = 0xFFFFFFFF                    # the device arrays of gofindthem_amd.group hold -1 behind the cap


def tag_ids(tags):
    ids = {}
    return [ids.setdefault(t, len(ids)) for t in tags]


def make_group(exprs, tags, schema=None, include=None, exclude=None, rules=None, regex=None):
    f = Finder(GpuEngine(), PyRegexpEngine() if regex else EmptyRgxEngine(), False)
    for e, t in zip(exprs, tags):
        f.AddExpressionWithTag(e, t)
    if regex:
        f.AddExpressionWithTag(*regex)
    g = group.NewFinderWithRules(f, rules or {})
    if schema is not None:
        g.SetSchema(schema, include, exclude)
    return g


def dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a).astype(dt)).cuda()


def host(got):
    """a device result -> numpy: (row_off, ent_field, ent_expr, ent_tag or None, total)"""
    return tuple(x.cpu().numpy() if hasattr(x, "cpu") else x for x in got)


def as_want(ref):
    """a result of gft_debug_tag_entries (uncapped) in the form tag_entries.assert_entries compares with"""
    row_off, ef, ee, _, total = ref
    return row_off, ef[:total], ee[:total], {"total": total}


class Case:
    """one (E, F) configuration: schema with an excluded field, finder expressions, a planted batch, the oracle's leaf bitmap"""

    def __init__(self, E, F=8, N=60, seed=0, max_leaves=4):
        rng = np.random.default_rng([seed, E, F])
        self.schema = R.make_schema(F)
        self.include, self.exclude = None, [self.schema[-1]] + ([self.schema[2]] if F > 4 else [])
        self.exprs, self.tags = R.make_expressions(E, 7, rng)
        self.exp = R.Expectation(self.exprs, self.tags, {}, self.schema, self.include, self.exclude)
        self.valid = TE.valid_fields(self.schema, self.include, self.exclude)
        self.records = TE.planted_records(N, self.schema, rng, self.valid, max_leaves)
        texts, self.field, self.rec_off = R.csr(self.records, self.schema)
        self.hits = self.exp.hit_bitmap(texts)
        self.E, self.expr_tag, self.rng = E, tag_ids(self.tags), rng
        self.g = make_group(self.exprs, self.tags, self.schema, self.include, self.exclude)

    def check(self, hits=None, field=None, rec_off=None, cap=None, want_tag=True, vacuous_ok=False):
        """the three launches == gft_debug_tag_entries, guard words included; returns the restatement's statistics"""
        hits = self.hits if hits is None else hits
        field = self.field if field is None else field
        rec_off = self.rec_off if rec_off is None else rec_off
        ref = self.g.debug_tag_entries(hits, self.E, field, rec_off)
        got = host(self.g.debug_tag_entries_device(dev(hits.view(np.int32), np.int32), self.E, dev(field, np.int32), dev(rec_off, np.int64),
                                                   cap=cap, want_tag=want_tag))
        TE.assert_entries(got, as_want(ref), self.expr_tag, cap=cap, guard=GUARD_DEV)
        stats = TE.expected(hits, self.E, field, rec_off, self.valid)[3]
        assert stats["total"] == ref[4]
        if not vacuous_ok:
            TE.assert_not_vacuous(stats)
        return stats


_cases = {}


def case(E, **kw):
    key = (E, tuple(sorted(kw.items())))
    if key not in _cases:
        _cases[key] = Case(E, **kw)
    return _cases[key]


def dirty(hits, E):
    """the rows with every bit at and above E set in the last word"""
    out = hits.copy()
    if E % 32:
        out[:, -1] |= np.uint32((0xFFFFFFFF << (E % 32)) & 0xFFFFFFFF)
        assert not np.array_equal(out, hits)
    return out


# ---- 1. the three launches over an oracle leaf bitmap ---------------------------------------------------------------------------
@pytest.mark.parametrize("EW", [1, 2, 3, 32, 33, 64, 65, 129])
def test_row_widths_clean_and_with_garbage_above_the_last_expression(EW):
    """EW = 3: a segment of four lanes with an idle lane; 65: the carry path; 129: three steps, the last one partial"""
    E = 32 * EW - 5
    c = case(E)
    assert c.hits.shape[1] == EW
    stats = c.check()
    assert c.check(hits=dirty(c.hits, E)) == stats


@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 129])
def test_record_counts(N):
    c = case(40, N=129)
    assert len(c.records) >= 129
    recs = c.records[:N]
    texts, field, rec_off = R.csr(recs, c.schema)
    c.check(c.hits[:len(field)], field, rec_off, vacuous_ok=N < 63)


def test_records_of_1_63_64_65_and_300_leaves():
    c = case(40)
    rng = np.random.default_rng(3)
    V = R.vocabulary()
    recs = []
    for n in (1, 63, 64, 65, 300, 1, 64):
        recs.append([(c.schema[int(rng.integers(len(c.schema)))], " ".join(V[int(x)] for x in rng.integers(0, len(V), int(rng.integers(0, 4)))))
                     for _ in range(n)])
    texts, field, rec_off = R.csr(recs, c.schema)
    c.check(c.exp.hit_bitmap(texts), field, rec_off)


def test_a_block_whose_only_contributing_leaf_is_its_last():
    """E = 40: two words a row, 32 leaves a wave and trip, four trips in flight, four waves: a block takes 512 leaves"""
    c = case(40)
    good = c.schema[0]
    assert c.valid[0]
    recs = [[(good, "")] * 3 for _ in range(170)] + [[(good, ""), (good, TE.EVERYTHING)]] + [[(good, "")] * 511 + [(good, TE.EVERYTHING)]]
    texts, field, rec_off = R.csr(recs, c.schema)
    assert len(field) == 1024
    hits = c.exp.hit_bitmap(texts)
    assert hits[511].any() and hits[1023].any() and not hits[:511].any() and not hits[512:1023].any()
    stats = c.check(hits, field, rec_off, vacuous_ok=True)
    assert stats["total"] > 0 and stats["silent"] == 1022


@pytest.mark.parametrize("n_leaves", [4095, 4096, 4097, 8193])
def test_leaf_counts_at_the_scan_tile(n_leaves):
    """the scan works in tiles of 4096 counts"""
    c = case(3)
    rng = np.random.default_rng(n_leaves)
    reps = -(-n_leaves // len(c.field))
    hits, field = np.tile(c.hits, (reps, 1))[:n_leaves], np.tile(c.field, reps)[:n_leaves]
    perm = rng.permutation(n_leaves)
    hits, field = np.ascontiguousarray(hits[perm]), field[perm]
    cuts = np.sort(rng.integers(0, n_leaves + 1, 700))
    rec_off = np.concatenate([[0], cuts, [n_leaves]]).astype(np.uint64)
    stats = c.check(hits, field, rec_off)
    assert stats["total"] > n_leaves // 64


def test_all_ones_rows_make_runs_longer_than_a_wave():
    c = case(1000)
    ones = np.full_like(c.hits, 0xFFFFFFFF)
    stats = c.check(ones, vacuous_ok=True)
    n_valid = sum(c.valid[int(f)] for f in c.field)
    assert stats["total"] == 1000 * n_valid and 0 < n_valid < len(c.field) and stats["masked"] > 0


@pytest.mark.parametrize("E", [40, 2075])
def test_caps_store_a_prefix_and_nothing_behind_it(E):
    c = case(E)
    total = c.check()["total"]
    assert total > 8
    for cap in (0, 1, total - 1, total, total + 7):
        c.check(cap=cap)
    c.check(cap=total - 1, want_tag=False)
    # NULL arrays with cap == 0 count only
    row_off, t = torch.zeros(len(c.rec_off), dtype=torch.int64, device="cuda"), C.c_uint64()
    h, f, ro = dev(c.hits.view(np.int32), np.int32), dev(c.field, np.int32), dev(c.rec_off, np.int64)
    torch.cuda.synchronize()
    L = _lib.load()
    assert L.gft_debug_tag_entries_device(c.g._h, h.data_ptr(), E, f.data_ptr(), ro.data_ptr(), len(c.rec_off) - 1, len(c.field),
                                          row_off.data_ptr(), None, None, None, 0, C.byref(t)) == 0
    assert t.value == total and int(row_off[-1]) == total
    assert L.gft_debug_tag_entries_device(c.g._h, h.data_ptr(), E, f.data_ptr(), ro.data_ptr(), len(c.rec_off) - 1, len(c.field),
                                          row_off.data_ptr(), None, None, None, 3, C.byref(t)) == _lib.GFT_E_INVALID


@pytest.mark.parametrize("E", [40, 2075])
def test_invalid_batches_are_refused_and_the_handle_answers(E):
    c = case(E)
    bad_field = c.field.copy()
    bad_field[len(c.field) // 2] = len(c.schema)                          # a field index equal to n_fields
    k = int(np.flatnonzero(np.diff(c.rec_off.astype(np.int64)) > 0)[0])
    descending = c.rec_off.copy()
    descending[k], descending[k + 1] = c.rec_off[k + 1], c.rec_off[k]
    beyond = c.rec_off.copy()
    beyond[len(beyond) // 2:] += np.uint64(1 << 40)                       # leaves [0, n_leaves]: never used as an index
    h = dev(c.hits.view(np.int32), np.int32)
    for field, rec_off, word in [(bad_field, c.rec_off, "field"), (c.field, descending, "rec_off"), (c.field, beyond, "rec_off")]:
        with pytest.raises(group.GroupFinderError) as ei:
            c.g.debug_tag_entries_device(h, E, dev(field, np.int32), dev(rec_off.astype(np.int64), np.int64))
        assert ei.value.code == _lib.GFT_E_INVALID and word in str(ei.value)
        c.check()
    with pytest.raises(group.GroupFinderError) as ei:                     # leaves but no records
        c.g.debug_tag_entries_device(h, E, dev(c.field, np.int32), dev(c.rec_off[-1:], np.int64))
    assert ei.value.code == _lib.GFT_E_INVALID
    c.check()


def test_no_expressions_no_leaves_no_records():
    g = make_group([], [], ["Field", "Other"])
    z = torch.zeros(0, dtype=torch.int32, device="cuda")
    row_off, ef, ee, et, total = host(g.debug_tag_entries_device(z, 0, dev([0, 1, 0], np.int32), dev([0, 1, 3], np.int64)))
    assert total == 0 and row_off.tolist() == [0, 0, 0] and (ef.astype(np.uint32) == GUARD_DEV).all()
    with pytest.raises(group.GroupFinderError) as ei:                     # the fields are checked all the same
        g.debug_tag_entries_device(z, 0, dev([0, 2, 0], np.int32), dev([0, 1, 3], np.int64))
    assert ei.value.code == _lib.GFT_E_INVALID
    c = case(40)
    c.check(c.hits[:0], c.field[:0], np.zeros(1, np.uint64), vacuous_ok=True)
    c.check(c.hits[:0], c.field[:0], np.zeros(4, np.uint64), vacuous_ok=True)


def test_one_cu_every_wave_takes_several_trips():
    """the engine held to one CU: 8 blocks, 32 waves; 20 000 leaves of two words are 157 groups of four trips"""
    c = case(40)
    reps = -(-20000 // len(c.field))
    hits, field = np.ascontiguousarray(np.tile(c.hits, (reps, 1))[:20000]), np.tile(c.field, reps)[:20000]
    rec_off = np.arange(0, 20001, 4, dtype=np.uint64)
    L, e = _lib.load(), c.g.findthem.engine_handle()
    assert e and L.gft_set_cu_margin(e, S.ONE_CU) == 0
    try:
        stats = c.check(hits, field, rec_off)
    finally:
        assert L.gft_set_cu_margin(e, 0) == 0
    assert stats["total"] > 20000
    wide = case(2075)                                                     # a wave a row: 32 waves, 1 000 rows
    reps = -(-1000 // len(wide.field))
    assert L.gft_set_cu_margin(wide.g.findthem.engine_handle(), S.ONE_CU) == 0
    try:
        wide.check(np.ascontiguousarray(np.tile(wide.hits, (reps, 1))[:1000]), np.tile(wide.field, reps)[:1000], np.arange(0, 1001, 5, dtype=np.uint64))
    finally:
        assert L.gft_set_cu_margin(wide.g.findthem.engine_handle(), 0) == 0


# ---- 2. the record calls ---------------------------------------------------------------------------------------------------------
def records_config(seed, include=None, exclude=None, regex=None, rules=True, lower=None):
    rng = np.random.default_rng([seed, 77])
    schema = R.make_schema(8)
    exprs, tags = R.make_expressions(40, 5, rng)
    rules = R.make_rules(12, 5, schema, rng) if rules else {}
    exp = R.Expectation(exprs, tags, rules, schema, include, exclude, lower=lower)
    return make_group(exprs, tags, schema, include, exclude, rules, regex), exp, rng


def device_entries(g, records, cap=None):
    blob, off, field, rec_off = g.pack_records(records)
    return host(g.TagRecordsDevice(dev(blob, np.uint8), dev(off, np.int64), dev(field, np.int32), dev(rec_off, np.int64), cap=cap))


def device_rule_rows(g, records):
    blob, off, field, rec_off = g.pack_records(records)
    out = g.ProcessRecordsDevice(dev(blob, np.uint8), dev(off, np.int64), dev(field, np.int32), dev(rec_off, np.int64))
    return out.cpu().numpy()


def test_scratch_reuse_and_growth_beside_the_rule_route():
    """a large batch, a small one, a larger one on one handle, a ProcessRecordsDevice of the same batch between the tag calls:
    its rows are those of a handle that never made a tag call"""
    g, exp, rng = records_config(1, exclude=[R.make_schema(8)[2]])
    clean, _, _ = records_config(1, exclude=[R.make_schema(8)[2]])
    valid = TE.valid_fields(exp.schema, None, exp.exclude)
    for n in (1500, 20, 4000):
        recs = TE.planted_records(n, exp.schema, rng, valid)
        texts, field, rec_off = R.csr(recs, exp.schema)
        want = TE.expected(exp.hit_bitmap(texts), 40, field, rec_off, valid)
        TE.assert_not_vacuous(want[3])
        TE.assert_entries(device_entries(g, recs), want, tag_ids(exp.tags), guard=GUARD_DEV)
        rows = device_rule_rows(g, recs)
        assert np.array_equal(rows, device_rule_rows(clean, recs)) and rows.any()
        TE.assert_entries(device_entries(g, recs), want, tag_ids(exp.tags), guard=GUARD_DEV)


@pytest.mark.parametrize("include,exclude", [(None, None), (["G0", "G1"], ["G0.b"]), (None, ["G1", "G0.a"])])
def test_tag_records_device_and_both_host_routes_against_the_oracle(include, exclude):
    g, exp, rng = records_config(2, include, exclude, rules=False)
    g_rx, _, _ = records_config(2, include, exclude, regex=(r'r"zq+x[0-9]"', "rxtag"), rules=False)
    assert g_rx.findthem.GetRegexes()
    valid = TE.valid_fields(exp.schema, include, exclude)
    recs = TE.planted_records(130, exp.schema, rng, valid)
    texts, field, rec_off = R.csr(recs, exp.schema)
    hits = exp.hit_bitmap(texts)
    want = TE.expected(hits, 40, field, rec_off, valid)
    TE.assert_not_vacuous(want[3], masked=exclude is not None or include is not None)
    maps = TE.tag_maps(exp, recs, hits)
    ids = tag_ids(exp.tags)
    got = device_entries(g, recs)
    TE.assert_entries(got, want, ids, guard=GUARD_DEV)
    assert g.tags_from_entries(got[0], got[1][:got[4]], got[2][:got[4]]) == maps
    arrays = g.pack_records(recs)
    for grp in (g, g_rx):                                                 # the device route, the host route: the same arrays
        TE.assert_entries(grp.TagRecordsEntries(*arrays), want, ids + [5])
        for cap in (0, 1, want[3]["total"] - 1, want[3]["total"] + 7):
            TE.assert_entries(grp.TagRecordsEntries(*arrays, cap=cap), want, ids + [5], cap=cap)
        assert grp.TagRecords(recs) == maps
    with pytest.raises(group.GroupFinderError) as ei:                     # the device-pointer call needs the device route
        device_entries(g_rx, recs)
    assert ei.value.code == _lib.GFT_E_UNSUPPORTED
    assert sum(len(m) for m in maps) > 50


def test_non_ascii_upper_case_leaves_are_lowered_on_the_device():
    exprs = ['"école"', '"ecole" or "straße"', '"kelvin"', '"istanbul"', 'inord("la" and "carte")']
    tags = ["fr", "mixed", "unit", "city", "menu"]
    schema = ["Title", "Body", "Body.note"]
    texts = ["Vive la École", "LA STRASSE École", "à LA CARTE", "273 Kelvin", "İstanbul", "plain", ""]
    recs = [[(schema[(r + k) % 3], texts[(r * 3 + k) % len(texts)]) for k in range(r % 4)] for r in range(90)]
    exclude = ["Body.note"]
    exp = R.Expectation(exprs, tags, {}, schema, None, exclude, lower=ref_lower)
    g = make_group(exprs, tags, schema, None, exclude)
    valid = TE.valid_fields(schema, None, exclude)
    _, field, rec_off = R.csr(recs, schema)
    hits = exp.hit_bitmap([t for rec in recs for _, t in rec])
    want = TE.expected(hits, 5, field, rec_off, valid)
    TE.assert_not_vacuous(want[3])
    before = g.findthem.lowered_batches()
    cap = want[3]["total"] + 5                                             # (a cap given: one call, one batch through the finder)
    TE.assert_entries(device_entries(g, recs, cap=cap), want, tag_ids(tags), cap=cap, guard=GUARD_DEV)
    assert g.findthem.lowered_batches() == (before[0] + 1, before[1])
    assert g.TagRecords(recs) == TE.tag_maps(exp, recs, hits)
    ascii_only = R.Expectation(exprs, tags, {}, schema, None, exclude).hit_bitmap([t for rec in recs for _, t in rec])
    assert not np.array_equal(hits, ascii_only), "the batch does not need strings.ToLower"


def test_refusals_of_the_record_calls_leave_the_handle_answering():
    g, exp, rng = records_config(3)
    recs = R.make_records(66, exp.schema, rng)
    blob, off, field, rec_off = g.pack_records(recs)
    want = device_entries(g, recs)
    bad_field = field.copy(); bad_field[len(field) // 2] = len(exp.schema)
    descending = rec_off.copy(); descending[10], descending[11] = rec_off[11] + 1, rec_off[10]
    for f, ro in [(bad_field, rec_off), (field, descending)]:
        with pytest.raises(group.GroupFinderError) as ei:
            g.TagRecordsEntries(blob, off, f, ro)
        assert ei.value.code == _lib.GFT_E_INVALID
        with pytest.raises(group.GroupFinderError) as ei:
            g.TagRecordsDevice(dev(blob, np.uint8), dev(off, np.int64), dev(f, np.int32), dev(ro, np.int64))
        assert ei.value.code == _lib.GFT_E_INVALID
        again = device_entries(g, recs)
        assert all(np.array_equal(a, b) for a, b in zip(again[:4], want[:4])) and again[4] == want[4] > 0
    with pytest.raises(group.GroupFinderError) as ei:
        group.NewFinder(g.findthem).TagRecordsDevice(dev(blob, np.uint8), dev(off, np.int64), dev(field, np.int32), dev(rec_off, np.int64))
    assert ei.value.code == _lib.GFT_E_INVALID and "schema" in str(ei.value)


def test_profile_names_the_three_launches():
    g, exp, rng = records_config(4)
    recs = R.make_records(64, exp.schema, rng)
    device_entries(g, recs)
    L, e = _lib.load(), g.findthem.engine_handle()
    assert L.gft_profile_enable(e, 1) == 0
    try:
        device_entries(g, recs, cap=100000)
        for name in (b"tags_count", b"tags_scan", b"tags_fill"):
            ms, n = C.c_double(), C.c_uint64()
            assert L.gft_profile_read(e, name, C.byref(ms), C.byref(n)) == 0
            assert n.value == 1 and ms.value > 0
    finally:
        L.gft_profile_reset(e)
        L.gft_profile_enable(e, 0)


# ---- 3. the JSON calls -----------------------------------------------------------------------------------------------------------
def test_tag_jsons_device_equals_the_record_route():
    g, exp, rng = records_config(5, exclude=[R.make_schema(8)[2]])
    docs = [J.gen_doc(exp.schema, rng, R.vocabulary()) for _ in range(200)]
    got, status = g.TagJsonsDevice(*to_device(docs))
    got, status = host(got), status.cpu().numpy()
    records = [R.flatten(json.loads(d.decode("utf-8"))) for d in docs]
    want = device_entries(g, records)
    assert not status.any() and got[4] == want[4] > 0
    assert all(np.array_equal(a, b) for a, b in zip(got[:4], want[:4]))
    maps = g.tags_from_entries(got[0], got[1][:got[4]], got[2][:got[4]])
    assert maps == [r["tags"] for r in g.TagJsons(docs, None, exp.exclude)]
    # a document that is handed back has an empty row; the cap protocol holds here too
    (row_off, ef, ee, et, total), status2 = g.TagJsonsDevice(*to_device([docs[0], b'{"nosuch":"x"}', b"{", docs[1]]), cap=3)
    row_off = row_off.cpu().numpy()
    assert status2.cpu().tolist() == [0, J.PATH, J.SYNTAX, 0]
    assert row_off[1] == row_off[2] == row_off[3] and row_off[1] == got[0][1] and row_off[4] - row_off[3] == got[0][2] - got[0][1] and total == row_off[4]
    n = min(3, total)
    assert np.array_equal(ee.cpu().numpy()[:n], got[2][:n]) and (ee.cpu().numpy()[3:] == -1).all()


TABLE_EXPRS = ['"x"', '"y"', '"v"', '"lorem" and "ipsum"', '"p"', '"s" or "q"', '"first"', 'inord("lorem" and "ipsum")', '"é"', '"w"']
TABLE_TAGS = ["t0", "t1", "t0", "t2", "t1", "t2", "t0", "t3", "t3", "t1"]


@pytest.mark.parametrize("schema", [J.SCHEMA, J.SCHEMA_UTF8, J.deep_schema(32), J.deep_schema(33)], ids=["default", "utf8", "deep32", "deep33"])
def test_tag_jsons_schema_on_the_table(schema):
    """every document of tests/json_docs.py's table: those with status 0 take their entries, all others come back through the host
    route with their tags or their error"""
    docs = [d for d in J.table() if d.schema == schema]
    exclude = [schema[3]] if len(schema) > 3 else None
    g = make_group(TABLE_EXPRS, TABLE_TAGS, schema, None, exclude)
    raws = [d.raw for d in docs]
    want = g.TagJsons(raws, None, exclude)
    got = g.TagJsonsSchema(raws)
    assert got == want
    n_host = sum(d.status != 0 for d in docs)
    assert g.json_last() == (len(docs) - n_host, n_host)
    if schema is J.SCHEMA:
        handed_back = [r for d, r in zip(docs, got) if d.status != 0]
        assert any(r.get("tags") for r in handed_back) and any("error" in r for r in handed_back)
        assert sum(1 for d, r in zip(docs, got) if d.status == 0 and r.get("tags")) > 5
    assert g.TagJsonsSchema([]) == [] and g.json_last() == (0, 0)


def test_tag_jsons_schema_on_2000_generated_documents():
    rng = np.random.default_rng(42)
    schema = R.make_schema(8)
    exprs, tags = R.make_expressions(40, 5, rng)
    include, exclude = [schema[0], schema[1], schema[5]], [schema[1]]
    g = make_group(exprs, tags, schema, include, exclude)
    docs = []
    for _ in range(2000):
        d = J.gen_doc(schema, rng, R.vocabulary())
        docs.append(J.mutate(d, rng) if rng.random() < 0.1 else d)
    want = g.TagJsons(docs, include, exclude)
    assert g.TagJsonsSchema(docs) == want
    n_device, n_host = g.json_last()
    assert n_device + n_host == 2000 and n_device > 1700 and n_host > 0
    assert sum(1 for r in want if r.get("tags")) > 300 and any("error" in r for r in want) and any(r.get("tags") == {} for r in want)
    # a regex finder takes the host route for the whole batch
    g_rx = make_group(exprs, tags, schema, include, exclude, regex=(r'r"zq+x[0-9]"', "rxtag"))
    assert g_rx.TagJsonsSchema(docs[:100]) == want[:100] and g_rx.json_last() == (0, 100)
    with pytest.raises(group.GroupFinderError) as ei:
        g_rx.TagJsonsDevice(*to_device(docs[:3]))
    assert ei.value.code == _lib.GFT_E_UNSUPPORTED


def nested_config(seed):
    """the finder and documents of test_gpu_group.py's generated-documents test: nested objects with lists"""
    from gofindthem_amd.workload import Workload, make_expressions
    from test_gpu_group import _random_docs
    rng = np.random.default_rng(seed)
    w = Workload(300)
    exprs = make_expressions(w.terms(), 60, inord_fraction=0.3)
    tags = ["tag%d" % (i % 7) for i in range(len(exprs))]
    g = make_group(exprs, tags, rules={"r": ['"tag0" and "tag1:Body"']})
    return g, [json.dumps(d) for d in _random_docs(rng, w, 100)]


def test_tag_jsons_auto_on_nested_documents_with_lists():
    g, raws = nested_config(0)
    want = g.TagJsons(raws)
    assert g.TagJsonsAuto(raws) == want and g.json_last() == (100, 0)
    n_paths, dropped, recompiled = g.json_auto_last()
    assert n_paths > 20 and dropped == 0 and recompiled == 1
    assert sum(1 for r in want if r.get("tags")) > 20
    for inc, exc in [(["Body", "Meta"], None), (None, ["Meta.Notes", "items"])]:
        assert g.TagJsonsAuto(raws, inc, exc) == g.TagJsons(raws, inc, exc) and g.json_last() == (100, 0)
    assert g.TagJsonsAuto([]) == [] and g.json_last() == (0, 0)
    # one kept schema serves the rule call and the tag call
    assert g.ProcessJsonsAuto(raws) == g.ProcessJsons(raws) and g.json_auto_last()[2] == 1
    assert g.TagJsonsAuto(raws) == want and g.json_auto_last()[2] == 0


def test_tag_jsons_auto_on_a_dropped_path_and_a_refused_schema():
    import json_paths_cases as P
    g, raws = nested_config(1)
    doc, paths = P.pool_overflow_doc()
    users = [b'{"' + p.replace(b".", b'":{"') + b'":"' + raws[i][2:40].encode().replace(b'"', b" ").replace(b"\\", b" ") + b'"}}}' for i, p in enumerate(paths[-6:])]
    docs = [r.encode() for r in raws[:40]] + [doc] + users
    got = g.TagJsonsAuto(docs)
    assert got == g.TagJsons(docs) and not any("error" in r for r in got)
    n_device, n_host = g.json_last()
    assert g.json_auto_last()[1] > 0 and n_host > 0 and n_device >= 40 and n_device + n_host == len(docs)
    # a schema beyond the trie's limit is never the caller's error: the host route for the whole batch
    docs = raws[:10] + [P.many_strings(P.PATH_CAP).decode()]
    assert g.TagJsonsAuto(docs) == g.TagJsons(docs) and g.json_last() == (0, 11)
    assert g.TagJsonsAuto(raws) == g.TagJsons(raws) and g.json_last() == (100, 0)


def test_tag_jsons_auto_beside_set_schemas_own_schema():
    rng = np.random.default_rng(8)
    schema = R.make_schema(8)
    exprs, tags = R.make_expressions(40, 5, rng)
    g = make_group(exprs, tags, schema, None, [schema[2]], rules=R.make_rules(20, 5, schema, rng))
    V = R.vocabulary()
    mine = [J.gen_doc(schema, rng, V) for _ in range(100)]
    want_mine = g.TagJsons(mine, None, [schema[2]])
    other = [json.dumps({"Other": {"deep": V[i % len(V)]}, "G0": [V[(i + 1) % len(V)], {"z": V[(i + 2) % len(V)]}]}) for i in range(50)]
    want_other = g.TagJsons(other)
    for _ in range(2):
        assert g.TagJsonsAuto(other) == want_other and g.json_last() == (50, 0)
        assert g.TagJsonsSchema(mine) == want_mine and g.json_last() == (100, 0)
        assert g.ProcessJsonsSchema(mine) == g.ProcessJsons(mine, None, [schema[2]])
    assert sum(1 for r in want_mine if r.get("tags")) > 10 and sum(1 for r in want_other if r.get("tags")) > 10
