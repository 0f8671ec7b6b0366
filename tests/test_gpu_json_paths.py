"""Path discovery on the device (csrc/gft_json.hip: k_json_paths) and ProcessJsonsAuto on top of it.  D, the set the device
returns, against E, the discovery mode of the same walker run on the host, and R, the reference of gft_debug_json_paths_ref, both
computed here through the debug calls: D == E always; R is a subset of D when nothing was dropped; D == R for documents of the
device class.  ProcessJsonsAuto against ProcessJsons as Python objects, whatever was dropped."""
import contextlib
import json

import numpy as np
import pytest
import torch  # noqa: F401  (before libgft.so is loaded: one HIP runtime)

import json_docs as J
import json_paths_cases as P
import records as R
import schema_scale as S
from gofindthem_amd import _lib, group
from gofindthem_amd.finder import EmptyRgxEngine, Finder, GpuEngine, PyRegexpEngine
from json_docs import to_device

pytestmark = pytest.mark.gpu

H = P.host_group()


def make_group(exprs, tags, rules, regex=None):
    f = Finder(GpuEngine(), PyRegexpEngine() if regex else EmptyRgxEngine(), False)
    for e, t in zip(exprs, tags):
        f.AddExpressionWithTag(e, t)
    if regex:
        f.AddExpressionWithTag(*regex)
    return group.NewFinderWithRules(f, rules)


_PLAIN = []


def plain():
    """a group whose finder has one expression, no rules and no schema: for the call that only discovers"""
    if not _PLAIN:
        _PLAIN.append(make_group(['"x"'], ["t"], {}))
    return _PLAIN[0]


@contextlib.contextmanager
def one_cu(g):
    """the engine of g on one CU: k_json_paths runs 8 blocks, 32 waves"""
    L, e = _lib.load(), g.findthem.engine_handle()
    assert e and L.gft_set_cu_margin(e, S.ONE_CU) == 0
    try:
        yield
    finally:
        assert L.gft_set_cu_margin(e, 0) == 0


def check(docs, g=None):
    """D == E, dropped included; sorted, each path once; R inside D when nothing was dropped.  Returns (D, dropped, R)"""
    got, dropped = (g or plain()).JsonPathsDevice(*to_device(docs))
    emu, emu_dropped, _ = H.debug_emulate_json_paths(docs)
    ref = H.debug_json_paths_ref(docs)
    assert got == emu and dropped == emu_dropped
    assert got == sorted(set(got))
    if not dropped:
        assert set(ref) <= set(got)
    return got, dropped, ref


TABLE = J.table()


def test_table_at_every_alignment():
    """the table documents shorter than 300 bytes (all but three) at the 64 alignments of their start in the blob, a neighbour glued
    behind each; the three long ones at eight alignments, for run time; R for the documents of the device class"""
    docs = [d for d in TABLE if len(d.raw) < 300]
    assert len(docs) > 120
    for align in range(64):
        batch = []
        for d in docs:
            batch += J.at_alignment(d.raw, align)
        check(batch)
    # the documents of 300 bytes and more (a few hundred to 66 508 bytes) at eight alignments, a piece border on either side
    long_docs = [d for d in TABLE if len(d.raw) >= 300]
    assert len(long_docs) >= 3
    batch = []
    for align in (0, 1, 7, 31, 32, 33, 62, 63):
        for d in long_docs:
            batch += J.at_alignment(d.raw, align)
    check(batch)
    # the whole table as one batch, and its device class alone
    check([d.raw for d in TABLE])
    in_class = [d.raw for d in TABLE if d.in_class]
    got, dropped, ref = check(in_class)
    assert got == ref and not dropped and len(got) > 10


def test_2000_documents_that_share_8_paths():
    docs, want = P.shared_paths_docs(2000)
    got, dropped, ref = check(docs)
    assert got == want == ref and dropped == 0


def test_a_wave_walks_dozens_of_documents():
    """one CU: 32 waves.  Deep key stacks in front of shallow documents: a stack entry that is not reset is a path no document has"""
    g = plain()
    g.JsonPathsDevice(*to_device(["{}"]))             # (the engine exists from here on)
    docs, want = P.shared_paths_docs(2000)
    deep = P.deep_then_shallow(1500)
    with one_cu(g):
        got, dropped, ref = check(docs)
        assert got == want and dropped == 0
        got, dropped, ref = check(deep)
        assert got == ref and dropped == 0 and 500 < len(got) < 8000
        rng = np.random.default_rng(3)
        mixed, clean = J.corpus(J.SCHEMA, rng, 1500)
        check(mixed)
    assert check(deep)[0] == got


def test_an_array_of_1000_strings():
    got, dropped, ref = check([P.many_strings(1000)])
    assert got == sorted(b"items.index(%d)" % i for i in range(1000)) == ref and dropped == 0


def test_path_cap():
    doc = P.many_strings(P.PATH_CAP + 1)
    got, dropped, ref = check([doc])
    assert len(got) == P.PATH_CAP and dropped >= 1 and len(ref) == P.PATH_CAP + 1 and set(got) <= set(ref)
    # many waves at the cap: which paths are kept depends on the order, how many does not
    docs = [P.many_strings(700, "k%d" % i) for i in range(30)]
    got, dropped = plain().JsonPathsDevice(*to_device(docs))
    assert len(got) == P.PATH_CAP and dropped == 30 * 700 - P.PATH_CAP and set(got) <= set(H.debug_json_paths_ref(docs)) and got == sorted(set(got))


def test_keys_of_63_to_4000_bytes_at_two_depths():
    docs, want = P.key_length_docs()
    got, dropped, ref = check(docs)
    assert got == want == ref and dropped == 0


def test_pool_overflow():
    """few paths of 60 000 bytes: more than the pool holds.  The paths that come back are whole -- what was written stayed inside
    the pool, whose last bytes they are -- and the engine's other buffers still answer"""
    doc, want = P.pool_overflow_doc()
    fit = P.pool_fit(want)
    got, dropped, ref = check([doc])
    assert got == sorted(want[:fit]) and dropped == len(want) - fit > 0 and ref == sorted(want)
    # several waves: the order differs, the paths are whole all the same
    docs = [doc.replace(b'"m', b'"w%d_' % i) for i in range(4)]
    got, dropped = plain().JsonPathsDevice(*to_device(docs))
    allowed = set(H.debug_json_paths_ref(docs))
    assert dropped > 0 and 100 < len(got) <= fit + 1 and set(got) <= allowed and len(got) + dropped == len(allowed)
    docs2, want2 = P.shared_paths_docs(50)
    assert check(docs2)[0] == want2


def test_edge_batches():
    g = plain()
    assert g.JsonPathsDevice(*to_device([])) == ([], 0)
    assert check(P.broken_docs())[2] == []
    assert check([b'"x"']) == ([b""], 0, [b""])
    check([b""])
    blob, off = to_device(['{"a":"x"}', "{}"])
    with pytest.raises(group.GroupFinderError) as e:
        g.JsonPathsDevice(blob, torch.flip(off, [0]))
    assert e.value.code == _lib.GFT_E_INVALID
    assert g.JsonPathsDevice(blob, off) == ([b"a"], 0)              # (the handle stays usable)


def test_profile_names_the_launch():
    g = plain()
    docs, _ = P.shared_paths_docs(100)
    g.JsonPathsDevice(*to_device(docs))
    L, e = _lib.load(), g.findthem.engine_handle()
    assert L.gft_profile_enable(e, 1) == 0
    try:
        g.JsonPathsDevice(*to_device(docs))
        ms, n = _lib.C.c_double(0), _lib.C.c_uint64(0)
        assert L.gft_profile_read(e, b"json_paths", _lib.C.byref(ms), _lib.C.byref(n)) == 0 and n.value == 1 and ms.value > 0
    finally:
        L.gft_profile_enable(e, 0)
        L.gft_profile_reset(e)


# ---- ProcessJsonsAuto == ProcessJsons ------------------------------------------------------------------------------------
def nested_config(seed, regex=None):
    """the finder, rules and documents of test_gpu_group.py's generated-documents test"""
    from gofindthem_amd.workload import Workload, make_expressions
    from test_gpu_group import _random_docs
    rng = np.random.default_rng(seed)
    w = Workload(300)
    exprs = make_expressions(w.terms(), 60, inord_fraction=0.3)
    tags = ["tag%d" % (i % 7) for i in range(len(exprs))]
    rules = {"r%d" % i: [r] for i, r in enumerate([
        '"tag0" and "tag1"', '"tag2:Body" or "tag3:Meta.Notes"', 'not "tag4" and ("tag5:items" or "tag6")',
        '"tag1:Title" and not "tag2:Body.index(0)"', '"tag0:Meta" or "tag0:Notes" or "tag0:Author"', 'not ("tag3" or "tag5")'])}
    g = make_group(exprs, tags, rules, regex)
    return g, [json.dumps(d) for d in _random_docs(rng, w, 100)], rng


@pytest.fixture(scope="module")
def nested():
    return nested_config(0)


def test_auto_on_100_nested_documents(nested):
    g, raws, _ = nested
    want = g.ProcessJsons(raws)
    assert g.ProcessJsonsAuto(raws) == want
    assert g.json_last() == (100, 0)
    n_paths, dropped, recompiled = g.json_auto_last()
    assert n_paths > 20 and dropped == 0 and recompiled == 1
    assert sum(1 for r in want if r.get("rules")) > 20
    assert g.ProcessJsonsAuto([]) == [] and g.json_last() == (0, 0)


def test_auto_with_include_and_exclude_lists(nested):
    g, raws, _ = nested
    for inc, exc in [(["Body", "Meta"], None), (None, ["Meta.Notes", "items"]), (g.GetFieldNames(), ["Body.index(1)"])]:
        assert g.ProcessJsonsAuto(raws, inc, exc) == g.ProcessJsons(raws, inc, exc)
        assert g.json_last() == (100, 0) and g.json_auto_last()[2] == 1          # (other lists: another schema)


def test_auto_with_non_ascii_upper_case_leaves(nested):
    """leaves that leave ASCII: the finder lowers the batch on the device and scans it again"""
    g, raws, _ = nested
    def shout(v):
        if isinstance(v, str):
            return v.upper() + " \u00c9\u00d6"
        if isinstance(v, dict):
            return {k: shout(x) for k, x in v.items()}
        return [shout(x) for x in v] if isinstance(v, list) else v
    docs = [json.dumps(shout(json.loads(r)), ensure_ascii=False) if i % 2 else r for i, r in enumerate(raws)]
    before = g.findthem.lowered_batches()[0]
    got = g.ProcessJsonsAuto(docs)
    assert g.findthem.lowered_batches()[0] > before
    assert got == g.ProcessJsons(docs) and not any("error" in r for r in got)
    assert g.json_last() == (100, 0)


def test_auto_when_paths_were_dropped(nested):
    """the pool overflows: the documents that use a path that was not kept take the host route, the result is the same"""
    g, raws, _ = nested
    doc, want = P.pool_overflow_doc()
    users = [b'{"' + p.replace(b".", b'":{"') + b'":"' + raws[i][2:40].encode().replace(b'"', b" ").replace(b"\\", b" ") + b'"}}}' for i, p in enumerate(want[-6:])]
    docs = [r.encode() for r in raws[:40]] + [doc] + users
    got = g.ProcessJsonsAuto(docs)
    assert got == g.ProcessJsons(docs) and not any("error" in r for r in got)
    n_device, n_host = g.json_last()
    n_paths, dropped, recompiled = g.json_auto_last()
    assert dropped > 0 and n_host > 0 and n_device >= 40 and n_device + n_host == len(docs) and recompiled == 1


def test_auto_with_duplicate_keys_and_surrogate_escapes(nested):
    g, raws, _ = nested
    docs = raws[:30] + ['{"Body":"first","Body":"%s"}' % raws[0][10:60].replace('"', " ").replace("\\", " "), '{"Title":"\\uD83D\\uDE00 x","Body":"\\uD83D"}',
                        '{"Meta":{"Notes":"a"},"Meta":"b"}', "{", '{"a\\u0062":"x"}', '{"":"y"}']
    got = g.ProcessJsonsAuto(docs)
    assert got == g.ProcessJsons(docs) and any("error" in r for r in got)
    n_device, n_host = g.json_last()
    assert n_device >= 30 and n_host >= 4 and n_device + n_host == len(docs)


def test_a_regex_finder_sends_the_batch_to_the_host():
    g, raws, _ = nested_config(1, regex=(r'r"zq+x[0-9]"', "rxtag"))
    assert g.ProcessJsonsAuto(raws) == g.ProcessJsons(raws)
    assert g.json_last() == (0, 100) and g.json_auto_last() == (0, 0, 0)


def test_a_schema_beyond_the_trie_limit_sends_the_batch_to_the_host(nested):
    g, raws, _ = nested
    docs = raws[:10] + [P.many_strings(P.PATH_CAP).decode()]           # 16384 paths: 16386 trie nodes
    assert g.ProcessJsonsAuto(docs) == g.ProcessJsons(docs)
    assert g.json_last() == (0, 11) and g.json_auto_last()[0] == P.PATH_CAP
    assert g.ProcessJsonsAuto(raws) == g.ProcessJsons(raws) and g.json_last() == (100, 0)


def test_the_two_schemas_do_not_disturb_each_other():
    rng = np.random.default_rng(8)
    schema = R.make_schema(8)
    exprs, tags = R.make_expressions(40, 5, rng)
    g = make_group(exprs, tags, R.make_rules(20, 5, schema, rng))
    g.SetSchema(schema)
    V = R.vocabulary()
    mine = [J.gen_doc(schema, rng, V) for _ in range(100)]
    records = R.make_records(60, schema, rng)
    want_docs, want_records = g.ProcessJsons(mine), g.ProcessRecords(records)
    assert g.ProcessJsonsSchema(mine) == want_docs and g.json_last() == (100, 0)
    other = [json.dumps({"Other": {"deep": V[i % len(V)]}, "G0": [V[(i + 1) % len(V)], {"z": V[(i + 2) % len(V)]}]}) for i in range(50)]
    for _ in range(2):
        assert g.ProcessJsonsAuto(other) == g.ProcessJsons(other) and g.json_last() == (50, 0)
        assert g.ProcessJsonsSchema(mine) == want_docs and g.json_last() == (100, 0)
        assert g.ProcessRecords(records) == want_records
    assert sum(1 for r in want_docs if r.get("rules")) > 10


def test_two_groups_on_one_finder_take_turns_with_json_batches():
    """one group with a schema, one that discovers its own, other rules, one engine: every call finds the other group's set and
    trie installed and puts its own back"""
    rng = np.random.default_rng(9)
    schema, shape = R.make_schema(8), R.make_schema(16)[8:]
    exprs, tags = R.make_expressions(40, 5, rng)
    g = make_group(exprs, tags, R.make_rules(20, 5, schema, rng))
    g.SetSchema(schema)
    g2 = group.NewFinderWithRules(g.findthem, R.make_rules(12, 5, shape, rng))
    V = R.vocabulary()
    mine = [J.gen_doc(schema, rng, V) for _ in range(100)]
    other = [J.gen_doc(shape, rng, V) for _ in range(50)]
    want, want2 = g.ProcessJsons(mine), g2.ProcessJsons(other)
    for turn in range(3):
        assert g.ProcessJsonsSchema(mine) == want and g.json_last() == (100, 0)
        assert g2.ProcessJsonsAuto(other) == want2 and g2.json_last() == (50, 0)
        assert g2.json_auto_last()[2] == (1 if turn == 0 else 0)
    assert min(sum(1 for r in res if r.get("rules")) for res in (want, want2)) > 10


def test_recompilation():
    g, _, _ = nested_config(2)
    V = R.vocabulary()
    docs = [json.dumps({"Body": V[i % len(V)], "Meta": {"Notes": V[(i + 3) % len(V)]}}) for i in range(40)]
    assert g.ProcessJsonsAuto(docs) == g.ProcessJsons(docs) and g.json_auto_last() == (2, 0, 1)
    assert g.ProcessJsonsAuto(docs[5:]) == g.ProcessJsons(docs[5:]) and g.json_auto_last() == (2, 0, 0)
    part = ['{"Body":"%s"}' % V[3], '{"Body":"x"}']                               # a subset of the kept paths
    assert g.ProcessJsonsAuto(part) == g.ProcessJsons(part) and g.json_auto_last() == (1, 0, 0)
    more = docs + ['{"Title":"%s"}' % V[0]]
    assert g.ProcessJsonsAuto(more) == g.ProcessJsons(more) and g.json_auto_last() == (3, 0, 1)
    assert g.ProcessJsonsAuto(docs) == g.ProcessJsons(docs) and g.json_auto_last() == (2, 0, 0)        # (the kept schema has them)
    g.AddRule("late", ['"tag1:Body" or "tag2:Title"'])
    assert g.ProcessJsonsAuto(more) == g.ProcessJsons(more) and g.json_auto_last() == (3, 0, 1) and g.json_last() == (41, 0)
    assert g.ProcessJsonsAuto(more) == g.ProcessJsons(more) and g.json_auto_last() == (3, 0, 0)
