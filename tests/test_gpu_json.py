"""JSON documents decoded on the device (csrc/gft_json.hip) into the record form, and the calls on top of it.  The kernels
against gft_debug_json_leaves_ref bit for bit -- the table of tests/json_docs.py at every alignment, generated and mutated
documents --; ProcessJsonsSchema against ProcessJsons as Python objects; ProcessJsonsDevice against ProcessRecordsDevice over
the records that tests/records.flatten makes of the same documents."""
import json

import numpy as np
import pytest
import torch  # noqa: F401  (before libgft.so is loaded: one HIP runtime)

import json_docs as J
import records as R
from json_docs import check_leaves, to_device
from gofindthem_amd import _lib, group
from gofindthem_amd.finder import EmptyRgxEngine, Finder, GpuEngine, PyRegexpEngine

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


_PLAIN = {}


def plain_group(schema):
    """a group whose finder has one expression and no rules: for the calls that only decode"""
    key = tuple(schema)
    if key not in _PLAIN:
        _PLAIN[key] = make_group(['"x"'], ["t"], {}, schema)
    return _PLAIN[key]


TABLE = J.table()
SCHEMAS = [J.SCHEMA, J.SCHEMA_UTF8, J.deep_schema(32), J.deep_schema(33)]


@pytest.mark.parametrize("schema", SCHEMAS, ids=["default", "utf8", "deep32", "deep33"])
def test_table(schema):
    docs = [d for d in TABLE if d.schema == schema]
    ref = check_leaves(plain_group(schema), [d.raw for d in docs])
    assert [int(s) for s in ref[0]] == [d.status for d in docs]


def test_table_at_every_alignment():
    """every piece-border document at every alignment 0..63 of its start in the blob, a neighbour glued behind it"""
    border = [d for d in TABLE if d.schema is J.SCHEMA and ("border" in d.name or "byte" in d.name)]
    assert len(border) > 30
    batch, want = [], []
    for d in border:
        for align in range(64):
            batch += J.at_alignment(d.raw, align)
            want += [J.SYNTAX, d.status, J.SYNTAX]
    ref = check_leaves(plain_group(J.SCHEMA), batch)
    assert [int(s) for s in ref[0]] == want


@pytest.fixture(scope="module")
def big():
    rng = np.random.default_rng(42)
    return J.corpus(J.SCHEMA, rng, 2000)


def test_generated_and_mutated_documents(big):
    docs, clean = big
    ref = check_leaves(plain_group(J.SCHEMA), docs)
    assert all(ref[0][i] == 0 for i in range(len(docs)) if clean[i]) and 100 < int((ref[0] != 0).sum()) and ref[5][0] > 2000


def test_batch_shapes(big):
    docs, _ = big
    g = plain_group(J.SCHEMA)
    check_leaves(g, [])
    for d in (docs[0], b"", b'"x"', TABLE[0].raw):
        check_leaves(g, [d])
    # the last document ends exactly at a piece border of the blob, and of its own
    head = docs[:7]
    fill = 64 - (sum(len(d) for d in head) + 2) % 64
    last = b'"' + b"q" * (fill + 64) + b'"'
    assert (sum(len(d) for d in head) + len(last)) % 64 == 0
    check_leaves(g, head + [last])
    check_leaves(g, [b'"' + b"q" * 62 + b'"'])
    check_leaves(g, [b'"' + b"q" * 126 + b'"'] * 3)


def test_caps(big):
    docs = big[0][:80]
    g = plain_group(J.SCHEMA)
    n_leaves, n_text = check_leaves(g, docs)[5]
    assert n_leaves > 20
    for caps in ((0, 0), (1, 7), (n_leaves - 1, n_text - 1), (n_leaves + 2, n_text + 2), (3, n_text), (n_leaves, 5)):
        check_leaves(g, docs, caps)


def test_refusals():
    g = plain_group(J.SCHEMA)
    blob, off = to_device(['{"a":"x"}', "{}"])
    with pytest.raises(group.GroupFinderError) as e:
        g.JsonLeavesDevice(blob, torch.flip(off, [0]))
    assert e.value.code == _lib.GFT_E_INVALID
    # the output over the input
    L = _lib.load()
    status = torch.zeros(2, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = L.gft_group_json_leaves_device(g._h, blob.data_ptr(), off.data_ptr(), 2, status.data_ptr(), off.data_ptr(), None, None, 0, None, 0, None)
    assert rc == _lib.GFT_E_INVALID and "overlaps" in str(g._err(rc))
    f = Finder(GpuEngine(), EmptyRgxEngine(), False)
    with pytest.raises(group.GroupFinderError) as e:
        group.NewFinder(f).JsonLeavesDevice(blob, off)
    assert e.value.code == _lib.GFT_E_INVALID and "schema" in str(e.value)
    check_leaves(g, ['{"a":"x"}', "{}"])             # (the handle stays usable)


# ---- the calls on top: rules ----------------------------------------------------------------------------------------------
def rules_config(seed, include=None, exclude=None, regex=None, F=8):
    rng = np.random.default_rng(seed)
    schema = R.make_schema(F)
    exprs, tags = R.make_expressions(40, 5, rng)
    rules = R.make_rules(20, 5, schema, rng)
    return make_group(exprs, tags, rules, schema, include, exclude, regex), schema, rng


def mixed_docs(schema, rng, n, words):
    docs, clean = [], []
    for _ in range(n):
        d = J.gen_doc(schema, rng, words)
        bad = rng.random() < 0.1
        docs.append(J.mutate(d, rng) if bad else d)
        clean.append(not bad)
    return docs, clean


def test_process_jsons_schema_with_include_and_exclude():
    schema = R.make_schema(8)
    g, schema, rng = rules_config(1, include=[schema[0], schema[5]], exclude=[schema[2]])
    docs, clean = mixed_docs(schema, rng, 300, R.vocabulary())
    want = g.ProcessJsons(docs, [schema[0], schema[5]], [schema[2]])
    assert g.ProcessJsonsSchema(docs) == want
    n_device, n_host = g.json_last()
    assert n_device + n_host == 300 and n_device >= sum(clean) > 200
    assert 20 < sum(1 for r in want if r.get("rules")) and any("error" in r for r in want)
    assert g.ProcessJsonsSchema([]) == [] and g.json_last() == (0, 0)


def test_process_jsons_schema_non_ascii_upper_case():
    """leaves that leave ASCII: the finder lowers the batch on the device and scans it again"""
    g, schema, rng = rules_config(2)
    words = [w.upper() + "É" if i % 3 == 0 else w for i, w in enumerate(R.vocabulary())] + ["ÀÖ"]
    docs, clean = mixed_docs(schema, rng, 300, words)
    before = g.findthem.lowered_batches()[0]
    got = g.ProcessJsonsSchema(docs)
    assert g.findthem.lowered_batches()[0] > before
    assert got == g.ProcessJsons(docs)
    assert g.json_last()[0] >= sum(clean)
    assert 20 < sum(1 for r in got if r.get("rules"))


def test_process_jsons_schema_with_a_regex_term_takes_the_host_route():
    g, schema, rng = rules_config(3, regex=(r'r"zq+x[0-9]"', "rxtag"))
    docs, _ = mixed_docs(schema, rng, 300, R.vocabulary())
    assert g.ProcessJsonsSchema(docs) == g.ProcessJsons(docs)
    assert g.json_last() == (0, 300)
    with pytest.raises(group.GroupFinderError) as e:
        g.ProcessJsonsDevice(*to_device(docs[:3]))
    assert e.value.code == _lib.GFT_E_UNSUPPORTED


def device_rows(g, schema, docs):
    """(ProcessJsonsDevice rows, status) and the ProcessRecordsDevice rows of what flatten() makes of the same documents"""
    rows, status = g.ProcessJsonsDevice(*to_device(docs))
    records = [R.flatten(json.loads(d.decode("utf-8"))) for d in docs]
    blob, off, field, rec_off = g.pack_records(records)
    dev = lambda a, dt: torch.from_numpy(a.astype(dt)).cuda()
    want = g.ProcessRecordsDevice(dev(blob, np.uint8), dev(off, np.int64), dev(field, np.int32), dev(rec_off, np.int64))
    return rows.cpu().numpy(), status.cpu().numpy(), want.cpu().numpy()


def test_process_jsons_device_equals_the_record_route():
    g, schema, rng = rules_config(4)
    docs = [J.gen_doc(schema, rng, R.vocabulary()) for _ in range(200)]
    rows, status, want = device_rows(g, schema, docs)
    assert not status.any() and np.array_equal(rows, want) and 0 < int((rows != 0).any(axis=1).sum())
    # a document that is handed back has the row of an empty record
    rows2, status2 = g.ProcessJsonsDevice(*to_device([docs[0], b'{"nosuch":"x"}', b"{", docs[1]]))
    empty = g.ProcessJsonsDevice(*to_device([b"{}"]))[0].cpu().numpy()[0]
    rows2 = rows2.cpu().numpy()
    assert status2.cpu().tolist() == [0, J.PATH, J.SYNTAX, 0]
    assert np.array_equal(rows2[0], want[0]) and np.array_equal(rows2[3], want[1]) and np.array_equal(rows2[1], empty) and np.array_equal(rows2[2], empty)


def test_growth_of_the_engine_buffers():
    """a fresh engine: the first call grows the record arrays, the second reuses them; then a larger batch grows them again"""
    g, schema, rng = rules_config(5)
    small = [J.gen_doc(schema, rng, R.vocabulary()) for _ in range(20)]
    large = [J.gen_doc(schema, rng, R.vocabulary()) for _ in range(600)]
    for docs in (small, small, large, large, small):
        rows, status, want = device_rows(g, schema, docs)
        assert not status.any() and np.array_equal(rows, want)
    assert g.last_batch()[0] == sum(len(R.flatten(json.loads(d.decode("utf-8")))) for d in small)


def test_records_of_64_leaves_across_a_rule_block_border():
    """65 documents of 64 leaves each: a k_record_rules block border falls inside the batch"""
    rng = np.random.default_rng(6)
    schema = ["f%d" % i for i in range(64)]
    exprs, tags = R.make_expressions(40, 5, rng)
    rules = R.make_rules(12, 5, schema, rng)
    g = make_group(exprs, tags, rules, schema)
    V = R.vocabulary()
    docs = [json.dumps({p: " ".join(V[int(x)] for x in rng.integers(0, len(V), 3)) for p in schema}).encode() for _ in range(65)]
    rows, status, want = device_rows(g, schema, docs)
    assert not status.any() and np.array_equal(rows, want) and g.last_batch()[0] == 65 * 64
    assert g.ProcessJsonsSchema(docs) == g.ProcessJsons(docs) and g.json_last() == (65, 0)
