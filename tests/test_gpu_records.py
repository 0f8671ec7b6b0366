"""The record form of the group finder on the GPU: leaves through the finder's device path, k_leaf_tags and k_record_rules
(csrc/gft_rules.hip) behind it.  Every comparison is bit for bit against oracle/group_ref.py's evaluate_rules over the CPU
oracle's ProcessText of every leaf (tests/records.py)."""
import json

import numpy as np
import pytest
import torch  # noqa: F401  (before libgft.so is loaded: one HIP runtime)

import records as R
from gofindthem_amd import _lib, group
from gofindthem_amd.finder import EmptyRgxEngine, Finder, GpuEngine, PyRegexpEngine
from tolower_cases import ref_lower

pytestmark = pytest.mark.gpu


def make_group(exprs, tags, rules, schema, include=None, exclude=None, regex=None):
    f = Finder(GpuEngine(), PyRegexpEngine() if regex else EmptyRgxEngine(), False)
    for e, t in zip(exprs, tags):
        f.AddExpressionWithTag(e, t)
    if regex:
        f.AddExpressionWithTag(*regex)
    g = group.NewFinderWithRules(f, rules)
    g.SetSchema(schema, include, exclude)
    return g


def config(seed, E=40, T=5, F=8, Rn=12, include=None, exclude=None):
    rng = np.random.default_rng([seed, E, T, F, Rn])
    schema = R.make_schema(F)
    exprs, tags = R.make_expressions(E, T, rng)
    rules = R.make_rules(Rn, T, schema, rng)
    exp = R.Expectation(exprs, tags, rules, schema, include, exclude)
    return make_group(exprs, tags, rules, schema, include, exclude), exp, rng


def device_rows(g, records):
    blob, off, field, rec_off = g.pack_records(records)
    dev = lambda a, dt: torch.from_numpy(a.astype(dt)).cuda()
    out = g.ProcessRecordsDevice(dev(blob, np.uint8), dev(off, np.int64), dev(field, np.int32), dev(rec_off, np.int64))
    return out.cpu().numpy().astype(np.uint32).reshape(len(records), g.rule_words())


def check(g, exp, records):
    want = exp.expected(records)
    got = g.ProcessRecordsBitmap(*g.pack_records(records))
    assert g.rule_exprs() == exp.numbering
    assert np.array_equal(got, want)
    return want


@pytest.fixture(scope="module")
def base():
    g, exp, rng = config(0)
    return g, exp, R.make_records(129, exp.schema, rng)


@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 129])
def test_record_counts_at_the_block_borders(base, N):
    g, exp, recs = base
    want = check(g, exp, recs[:N])
    assert np.array_equal(device_rows(g, recs[:N]), want)
    if N:
        planted = [[] if i in (0, 63, 64, N - 1) else r for i, r in enumerate(recs[:N])]
        want = check(g, exp, planted)
        assert 0 < int(want.any(axis=1).sum()) or N == 1
        assert np.array_equal(want[0], exp.expected([[]])[0])


@pytest.mark.parametrize("E,T,F,Rn", [(31, 3, 4, 5), (32, 3, 4, 5), (33, 3, 4, 5), (40, 1, 4, 5), (40, 32, 4, 5), (40, 33, 4, 5),
                                      (40, 5, 1, 5), (40, 5, 32, 5), (40, 5, 33, 5), (40, 5, 65, 5),
                                      (40, 5, 8, 1), (40, 5, 8, 32), (40, 5, 8, 33), (40, 5, 8, 65), (40, 5, 8, 300)])
def test_word_borders(E, T, F, Rn):
    g, exp, rng = config(1, E, T, F, Rn, exclude=None if F < 4 else [R.make_schema(F)[2]])
    recs = R.make_records(70, exp.schema, rng)
    want = check(g, exp, recs)
    true = int(np.unpackbits(want.view(np.uint8)).sum())
    assert 0 < true < 70 * Rn or Rn == 1


@pytest.mark.parametrize("E", [31, 32, 33])
def test_garbage_above_the_last_expression_is_ignored_by_the_kernels(E):
    """the two kernels over a caller-supplied device leaf bitmap (gft_debug_eval_rules_device): the oracle's rows with every bit
    at and above E set in a row's last word -- a kernel that read them would index past the expressions' tag ids"""
    g, exp, rng = config(4, E, 3, 4, 5)
    recs = R.make_records(70, exp.schema, rng)
    texts, field, rec_off = R.csr(recs, exp.schema)
    hits = exp.hit_bitmap(texts)
    want = exp.expected(recs, hits)
    dirty = hits.copy()
    if E % 32:
        dirty[:, -1] |= np.uint32((0xFFFFFFFF << (E % 32)) & 0xFFFFFFFF)
        assert not np.array_equal(dirty, hits)
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).cuda()
    for rows in (hits, dirty):
        got = g.debug_eval_rules_device(dev(rows.view(np.int32), np.int32), E, dev(field, np.int32), dev(rec_off, np.int64))
        assert np.array_equal(got.cpu().numpy().astype(np.uint32), want)
    assert 0 < int(np.unpackbits(want.view(np.uint8)).sum()) < 70 * 5


def test_uneven_blocks(base):
    g, exp, recs = base
    rng = np.random.default_rng(5)
    long = R.make_records(1, exp.schema, rng, max_leaves=1)[0]
    while len(long) < 200:
        long += R.make_records(1, exp.schema, rng, max_leaves=4)[0]
    small = R.make_records(150, exp.schema, rng, max_leaves=3)
    check(g, exp, small[:70] + [long[:200]] + small[70:])
    # a block whose only non-empty record is its last
    lone = [[]] * 63 + [small[1] or small[2] or [(exp.schema[0], R.A)]] + [[]] * 10
    want = check(g, exp, lone)
    assert np.array_equal(device_rows(g, lone), want)


@pytest.mark.parametrize("row", R.named_rows(), ids=lambda r: r[0])
def test_named_rows_end_to_end(row):
    _, exprs, tags, rules, schema, inc, exc, recs, want = row
    exp = R.Expectation(exprs, tags, rules, schema, inc, exc)
    g = make_group(exprs, tags, rules, schema, inc, exc)
    assert g.ProcessRecords(recs) == want
    check(g, exp, recs)


def test_both_routes_of_the_host_entry_point_agree():
    rng = np.random.default_rng(11)
    schema = R.make_schema(8)
    exprs, tags = R.make_expressions(40, 5, rng)
    rules = R.make_rules(20, 5, schema, rng)
    rules["rx"] = ['"rxtag" or "tag1"', 'not "rxtag:G0"']
    exp = R.Expectation(exprs, tags, rules, schema)
    recs = R.make_records(130, schema, rng)
    want = exp.expected(recs)                     # ("rxtag" is never matched: unknown to one finder, a regex without a match in the other)
    g_dev = make_group(exprs, tags, rules, schema)
    g_rx = make_group(exprs, tags, rules, schema, regex=(r'r"zq+x[0-9]"', "rxtag"))
    assert g_rx.findthem.GetRegexes()
    a = g_dev.ProcessRecordsBitmap(*g_dev.pack_records(recs))
    b = g_rx.ProcessRecordsBitmap(*g_rx.pack_records(recs))
    assert np.array_equal(a, want) and np.array_equal(b, want)
    # the device-pointer call needs the device route
    with pytest.raises(group.GroupFinderError) as ei:
        device_rows(g_rx, recs)
    assert ei.value.code == _lib.GFT_E_UNSUPPORTED
    assert np.array_equal(g_rx.ProcessRecordsBitmap(*g_rx.pack_records(recs[:5])), want[:5])


def test_non_ascii_batches_are_lowered_on_the_device():
    exprs = ['"école"', '"ecole" or "straße"', '"kelvin"', '"istanbul"', 'inord("la" and "carte")']
    tags = ["fr", "mixed", "unit", "city", "menu"]
    schema = ["Title", "Body", "Body.note"]
    rules = {"a": ['"fr:Body" or "city"', '"unit" and not "menu:Body"'], "b": ['"mixed:Title"', 'not "fr"']}
    texts = ["Vive la École", "LA STRASSE École", "à LA CARTE", "273 Kelvin", "İstanbul", "plain", ""]
    recs = [[(schema[(r + k) % 3], texts[(r * 3 + k) % len(texts)]) for k in range(r % 4)] for r in range(90)]
    exp = R.Expectation(exprs, tags, rules, schema, lower=ref_lower)
    g = make_group(exprs, tags, rules, schema)
    before = g.findthem.lowered_batches()
    want = check(g, exp, recs)
    assert g.findthem.lowered_batches() == (before[0] + 1, before[1])
    ascii_only = R.Expectation(exprs, tags, rules, schema).expected(recs)
    assert not np.array_equal(want, ascii_only), "the batch does not need strings.ToLower"


def test_device_tensors_equal_the_host_call(base):
    g, exp, recs = base
    assert np.array_equal(device_rows(g, recs), g.ProcessRecordsBitmap(*g.pack_records(recs)))
    assert g.ProcessRecords(recs[:20]) == exp.rules_of(recs[:20])[0]


def _random_docs(rng, n_docs):
    """the generator shape of test_gpu_group.py's documents, over this module's vocabulary"""
    V = R.vocabulary()
    keys = ["Title", "Body", "Meta", "Notes", "Author", "items"]

    def value(depth):
        r = rng.random()
        s = " ".join(V[int(x)] for x in rng.integers(0, len(V), int(rng.integers(0, 7))))
        if r < 0.45 or depth > 2:
            return s.upper() if rng.random() < 0.2 else s
        if r < 0.55:
            return [int(rng.integers(100)), None, True][int(rng.integers(3))]
        if r < 0.8:
            return [value(depth + 1) for _ in range(int(rng.integers(0, 4)))]
        return {kk: value(depth + 1) for kk in rng.choice(keys, int(rng.integers(1, 4)), replace=False)}
    return [{kk: value(0) for kk in rng.choice(keys, int(rng.integers(1, 6)), replace=False)} for _ in range(n_docs)]


def test_records_equal_process_jsons_on_flattened_documents():
    rng = np.random.default_rng(3)
    exprs, tags = R.make_expressions(60, 7, rng)
    rules = {"r%d" % i: [r] for i, r in enumerate([
        '"tag0" and "tag1"', '"tag2:Body" or "tag3:Meta.Notes"', 'not "tag4" and ("tag5:items" or "tag6")',
        '"tag1:Title" and not "tag2:Body.index(0)"', '"tag0:Meta" or "tag0:Notes" or "tag0:Author"', 'not ("tag3" or "tag5")'])}
    docs = _random_docs(rng, 100)
    recs = [R.flatten(d) for d in docs]
    schema = sorted({p for rec in recs for p, _ in rec})
    n_true = 0
    for inc, exc in [(None, None), (["Body", "Meta"], None), (None, ["Meta.Notes", "items"])]:
        g = make_group(exprs, tags, rules, schema, inc, exc)
        from_json = [r["rules"] for r in g.ProcessJsons([json.dumps(d) for d in docs], inc, exc)]
        assert g.ProcessRecords(recs) == from_json
        n_true += sum(len(d) for d in from_json)
    assert n_true > 100


def test_staleness_and_reuse():
    g, exp, rng = config(2)
    recs_a, recs_b = R.make_records(100, exp.schema, rng), R.make_records(70, exp.schema, rng)
    check(g, exp, recs_a)
    check(g, exp, recs_b)
    # a rule added between two batches: the numbering changes, the answers follow
    rules = {k: [raw for raw, _ in v] for k, v in exp.ref.rules.items()}
    g.AddRule("a_first", ['"tag1:G0" or not "tag2"'])
    rules["a_first"] = ['"tag1:G0" or not "tag2"']
    exp2 = R.Expectation(exp.exprs, exp.tags, rules, exp.schema)
    assert exp2.numbering[0][0] == "a_first" and exp2.numbering[1:] == exp.numbering
    check(g, exp2, recs_a)
    # a finder expression added: a new tag, known from now on
    g.AddRule("z_new", ['"fresh"', 'not "fresh:G0"'])
    rules["z_new"] = ['"fresh"', 'not "fresh:G0"']
    exp3 = R.Expectation(exp.exprs, exp.tags, rules, exp.schema)
    want3 = check(g, exp3, recs_b)
    g.findthem.AddExpressionWithTag('"%s"' % R.A, "fresh")
    exp4 = R.Expectation(exp.exprs + ['"%s"' % R.A], exp.tags + ["fresh"], rules, exp.schema)
    want4 = check(g, exp4, recs_b)
    assert not np.array_equal(want3, want4)
    assert np.array_equal(device_rows(g, recs_b), want4)


def test_two_groups_on_one_finder_keep_their_own_sets(base):
    g, exp, recs = base
    other_rules = {"only": ['not "tag0"', '"tag1:G1"']}
    g2 = group.NewFinderWithRules(g.findthem, other_rules)
    g2.SetSchema(exp.schema)
    exp2 = R.Expectation(exp.exprs, exp.tags, other_rules, exp.schema)
    for _ in range(2):
        check(g2, exp2, recs[:70])
        check(g, exp, recs[:70])


def test_two_groups_on_one_finder_from_two_threads(base):
    """a call holds the engine from the install of its set to the read of the flags: two groups with different rule sets, called
    concurrently, each get their own rows every time"""
    import threading
    g, exp, recs = base
    other_rules = {"only": ['not "tag0"', '"tag1:G1"', '"tag2" or "tag3:G0"']}
    g2 = group.NewFinderWithRules(g.findthem, other_rules)
    g2.SetSchema(exp.schema)
    exp2 = R.Expectation(exp.exprs, exp.tags, other_rules, exp.schema)
    jobs = [(g, g.pack_records(recs), exp.expected(recs)), (g2, g2.pack_records(recs[:70]), exp2.expected(recs[:70]))]
    bad = []

    def work(grp, arrays, want):
        try:
            for _ in range(20):
                if not np.array_equal(grp.ProcessRecordsBitmap(*arrays), want):
                    bad.append("rows differ")
        except Exception as x:          # noqa: BLE001 (reported below, on the main thread)
            bad.append(repr(x))
    threads = [threading.Thread(target=work, args=j) for j in jobs]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not bad, bad[:3]


def test_call_time_refusals_leave_the_handle_answering(base):
    g, exp, recs = base
    recs = recs[:66]
    blob, off, field, rec_off = g.pack_records(recs)
    want = exp.expected(recs)
    bad_field = field.copy(); bad_field[len(field) // 2] = len(exp.schema)
    descending = rec_off.copy(); descending[10], descending[11] = rec_off[11] + 1, rec_off[10]
    short = rec_off.copy(); short[-1] -= 1
    dev = lambda a, dt: torch.from_numpy(a.astype(dt)).cuda()
    for f, ro in [(bad_field, rec_off), (field, descending), (field, short)]:
        with pytest.raises(group.GroupFinderError) as ei:
            g.ProcessRecordsBitmap(blob, off, f, ro)
        assert ei.value.code == _lib.GFT_E_INVALID
        with pytest.raises(group.GroupFinderError) as ei:
            g.ProcessRecordsDevice(dev(blob, np.uint8), dev(off, np.int64), dev(f, np.int32), dev(ro, np.int64))
        assert ei.value.code == _lib.GFT_E_INVALID
        assert np.array_equal(g.ProcessRecordsBitmap(blob, off, field, rec_off), want)
    g0 = group.NewFinderWithRules(g.findthem, {"r": ['"tag0"']})
    with pytest.raises(group.GroupFinderError) as ei:
        g0.ProcessRecordsBitmap(blob, off, field, rec_off)
    assert ei.value.code == _lib.GFT_E_INVALID and "schema" in str(ei.value)
    # both routes refuse the same batches: leaves but no records; a bad field index under a group without rules
    for call in (lambda f, ro: g.ProcessRecordsBitmap(blob, off, f, ro),
                 lambda f, ro: g.ProcessRecordsDevice(dev(blob, np.uint8), dev(off, np.int64), dev(f, np.int32), dev(ro, np.int64))):
        with pytest.raises(group.GroupFinderError) as ei:
            call(field, rec_off[-1:])
        assert ei.value.code == _lib.GFT_E_INVALID
    g_norules = group.NewFinder(g.findthem)
    g_norules.SetSchema(exp.schema)
    for call in (lambda f: g_norules.ProcessRecordsBitmap(blob, off, f, rec_off),
                 lambda f: g_norules.ProcessRecordsDevice(dev(blob, np.uint8), dev(off, np.int64), dev(f, np.int32), dev(rec_off, np.int64))):
        with pytest.raises(group.GroupFinderError) as ei:
            call(bad_field)
        assert ei.value.code == _lib.GFT_E_INVALID
        assert tuple(call(field).shape) == (len(recs), 0)
    assert np.array_equal(device_rows(g, recs), want)


def test_profile_names(base):
    import ctypes as C
    g, exp, recs = base
    L, e = _lib.load(), g.findthem.engine_handle()
    assert L.gft_profile_enable(e, 1) == 0
    try:
        check(g, exp, recs[:64])
        for name in (b"group_tags", b"group_rules"):
            ms, n = C.c_double(), C.c_uint64()
            assert L.gft_profile_read(e, name, C.byref(ms), C.byref(n)) == 0
            assert n.value == 1 and ms.value > 0
    finally:
        L.gft_profile_reset(e)
        L.gft_profile_enable(e, 0)
