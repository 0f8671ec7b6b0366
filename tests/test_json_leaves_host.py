"""The device JSON walker without a device: gft_debug_emulate_json_leaves runs the source the kernels are compiled from
(csrc/gft_json_walk.hpp) on the host, 64-byte piece by piece, and must give what gft_debug_json_leaves_ref gives -- the host
route's JSON reader plus a walk of the decoded value, classified by code that shares nothing with the walker -- in status,
rec_off, leaf_field, leaf_off and text bytes.  The trie compiler (csrc/json_schema.cpp) is checked against a dict of the split
paths.  The same table and generators drive the kernels in test_gpu_json.py."""
import json

import numpy as np
import pytest

import json_docs as J
import records as R
from gofindthem_amd import _lib, finder, group


def _group(schema, rules=None):
    f = finder.Finder(None, None, False, allow_no_device=True)
    g = group.NewFinderWithRules(f, rules or {})
    g.SetSchema(schema)
    g._keep = f
    return g


_GROUPS = {}


def group_for(schema):
    key = tuple(schema)
    if key not in _GROUPS:
        _GROUPS[key] = _group(schema)
    return _GROUPS[key]


def same(a, b):
    """two results of the record form are equal in every array (behind the caps: untouched guard values on both sides)"""
    for x, y, what in zip(a[:5], b[:5], ("status", "rec_off", "leaf_field", "leaf_off", "text")):
        assert np.array_equal(x, y), what
    assert a[5] == b[5]


def test_symbols_exist():
    L = _lib.load()
    for name in ("gft_group_json_leaves_device", "gft_group_process_jsons_device", "gft_group_process_jsons_schema", "gft_group_json_last",
                 "gft_debug_json_leaves_ref", "gft_debug_emulate_json_leaves"):
        assert hasattr(L, name)


TABLE = J.table()


@pytest.mark.parametrize("doc", TABLE, ids=[d.name[:40] for d in TABLE])
def test_table_reference_and_walker(doc):
    """the expected status, on the reference side first; then the walker equals the reference; a document of status 0 holds the leaves
    that Python's json and the reference walk's flatten() give"""
    g = group_for(doc.schema)
    ref = g.debug_json_leaves_ref([doc.raw])
    assert int(ref[0][0]) == doc.status
    if doc.in_class:
        assert doc.status == J.OK
    emu = g.debug_emulate_json_leaves([doc.raw])
    same(emu, ref)
    if doc.status == J.OK:
        want = [(doc.schema.index(p), t.encode("utf-8")) for p, t in R.flatten(json.loads(doc.raw.decode("utf-8")))]
        assert J.leaves_of(*emu[:5])[0] == (0, want)
    else:
        assert emu[5] == (0, 0)


BORDER = [d for d in TABLE if "border" in d.name or "byte" in d.name or "bytes" in d.name]


def test_table_at_every_alignment():
    """every piece-border document at every alignment of its start, a neighbour glued behind it whose bytes would complete its last
    token: the walker reads no byte of the next document"""
    assert len(BORDER) > 30
    for doc in BORDER:
        g = group_for(doc.schema)
        alone = g.debug_json_leaves_ref([doc.raw])
        for align in range(64):
            batch = J.at_alignment(doc.raw, align)
            ref = g.debug_json_leaves_ref(batch)
            emu = g.debug_emulate_json_leaves(batch)
            same(emu, ref)
            assert int(emu[0][1]) == doc.status and J.leaves_of(*emu[:5])[1] == J.leaves_of(*alone[:5])[0]


def test_whole_table_as_one_batch():
    docs = [d for d in TABLE if d.schema is J.SCHEMA]
    g = group_for(J.SCHEMA)
    emu = g.debug_emulate_json_leaves([d.raw for d in docs])
    same(emu, g.debug_json_leaves_ref([d.raw for d in docs]))
    assert [int(s) for s in emu[0]] == [d.status for d in docs]


@pytest.mark.parametrize("seed,schema", [(1, J.SCHEMA), (2, R.make_schema(24)), (3, J.SCHEMA_UTF8 + J.SCHEMA)])
def test_random_documents(seed, schema):
    """generated from the schema (inside the device class by construction: asserted on the reference side first), mutated by one
    byte edit, random bytes"""
    rng = np.random.default_rng(seed)
    docs, clean = J.corpus(schema, rng, 400)
    g = group_for(schema)
    ref = g.debug_json_leaves_ref(docs)
    bad = [docs[i] for i in range(len(docs)) if clean[i] and ref[0][i] != 0]
    assert not bad, bad[:3]
    emu = g.debug_emulate_json_leaves(docs)
    same(emu, ref)
    got = J.leaves_of(*emu[:5])
    for i in range(len(docs)):
        if clean[i]:
            want = [(schema.index(p), t.encode("utf-8")) for p, t in R.flatten(json.loads(docs[i].decode("utf-8")))]
            assert got[i] == (0, want), docs[i]
    assert 0 < sum(1 for s in emu[0] if s) < len(docs) and emu[5][0] > 400


def test_mutations_of_the_table():
    """one byte edit of every table document, four times each"""
    rng = np.random.default_rng(7)
    docs = [J.mutate(d.raw, rng) for d in TABLE if d.schema is J.SCHEMA and len(d.raw) < 1000 for _ in range(4)]
    g = group_for(J.SCHEMA)
    same(g.debug_emulate_json_leaves(docs), g.debug_json_leaves_ref(docs))


def test_count_only_and_small_caps():
    rng = np.random.default_rng(11)
    docs, _ = J.corpus(J.SCHEMA, rng, 60)
    g = group_for(J.SCHEMA)
    full = g.debug_emulate_json_leaves(docs)
    n_leaves, n_text = full[5]
    assert n_leaves > 20 and n_text > 200
    L = _lib.load()
    for fn, name in ((L.gft_debug_emulate_json_leaves, "emulate"), (L.gft_debug_json_leaves_ref, "ref")):
        for leaf_cap, text_cap in ((0, 0), (1, 7), (n_leaves - 1, n_text - 1), (n_leaves, n_text), (n_leaves + 3, n_text + 3), (5, n_text), (n_leaves, 9)):
            got = g._json_leaves_host(fn, docs, leaf_cap, text_cap)
            assert got[5] == (n_leaves, n_text), name
            assert np.array_equal(got[0], full[0]) and np.array_equal(got[1], full[1])
            k = min(leaf_cap, n_leaves)
            assert np.array_equal(got[2][:k], full[2][:k]) and np.all(got[2][leaf_cap:] == 0xA5A5A5A5)
            end = k + 1 if n_leaves <= leaf_cap else k            # (leaf_off[n_leaves] is written when it lies inside the cap)
            assert np.array_equal(got[3][:end], full[3][:end]) and np.all(got[3][leaf_cap + 1:] == 0xA5A5A5A5A5A5A5A5)
            if n_leaves > leaf_cap:
                assert got[3][leaf_cap] == 0xA5A5A5A5A5A5A5A5
            t = min(text_cap, n_text)
            assert np.array_equal(got[4][:t], full[4][:t]) and np.all(got[4][text_cap:] == 0xA5)


def test_refusals():
    g = group.GroupFinder(finder.Finder(None, None, False, allow_no_device=True))
    with pytest.raises(group.GroupFinderError) as e:
        g.debug_emulate_json_leaves(["{}"])
    assert e.value.code == _lib.GFT_E_INVALID and "schema" in str(e.value)
    g = group_for(J.SCHEMA)
    L = _lib.load()
    blob = np.frombuffer(b"{}{}" + bytes(64), dtype=np.uint8)
    off = np.asarray([0, 4, 2], dtype=np.uint64)
    status, rec_off = np.zeros(2, dtype=np.uint8), np.zeros(3, dtype=np.uint64)
    for fn in (L.gft_debug_emulate_json_leaves, L.gft_debug_json_leaves_ref):
        assert fn(g._h, blob.ctypes.data, off.ctypes.data, 2, status.ctypes.data, rec_off.ctypes.data, None, None, 0, None, 0, None) == _lib.GFT_E_INVALID
        assert fn(g._h, blob.ctypes.data, off.ctypes.data, 0, None, rec_off.ctypes.data, None, None, 0, None, 0, None) == 0
        assert fn(g._h, blob.ctypes.data, off.ctypes.data, 1, status.ctypes.data, rec_off.ctypes.data, None, None, 3, None, 0, None) == _lib.GFT_E_INVALID


def test_trie_limits_are_refused_by_the_json_calls_only():
    many = ["p%d" % i for i in range(16384)]                      # 16384 nodes + the root
    g = _group(many)                                              # (the schema itself is accepted)
    with pytest.raises(group.GroupFinderError) as e:
        g.debug_emulate_json_leaves(["{}"])
    assert e.value.code == _lib.GFT_E_UNSUPPORTED and "16384" in str(e.value)
    with pytest.raises(group.GroupFinderError) as e:
        g.ProcessJsonsSchema(["{}"])
    assert e.value.code == _lib.GFT_E_UNSUPPORTED
    g = _group(many[:16383])
    assert int(g.debug_emulate_json_leaves(['{"p16382":"x"}'])[2][0]) == 16382
    g = _group(["a." + "k" * 65536])
    with pytest.raises(group.GroupFinderError) as e:
        g.debug_json_leaves_ref(["{}"])
    assert e.value.code == _lib.GFT_E_UNSUPPORTED and "65535" in str(e.value)
    g = _group(["a." + "k" * 65535])
    assert J.leaves_of(*g.debug_emulate_json_leaves(['{"a":{"%s":"v"}}' % ("k" * 65535)])[:5])[0] == (0, [(0, b"v")])


@pytest.mark.parametrize("schema", [J.SCHEMA, J.SCHEMA_UTF8, R.make_schema(40), ["x.y.z", "x.y", "x", "x.yy", "xy", "x..y", "index(1).index(10)"]])
def test_trie_lookups_against_a_dict(schema):
    g = _group(schema)
    nodes = {(): 0}                                               # tuple of components -> node
    want_field = {}
    for f, p in enumerate(schema):
        comps = tuple(p.split(".")) if p else ()
        want_field[comps] = f
        for k in range(1, len(comps) + 1):
            if comps[:k] not in nodes:
                if comps[k - 1] == "":
                    break                                         # an empty component is reached by no key (GFT_JSON_KEY)
                node, _ = g.debug_json_schema_find(nodes[comps[:k - 1]], comps[k - 1].encode("utf-8"))
                assert node > 0 and node not in nodes.values()
                nodes[comps[:k]] = node
    for comps, node in nodes.items():
        assert g.debug_json_schema_find(node, b"")[1] == want_field.get(comps, -1)
        for probe in ("", "nosuch", "index(0)", "x.y", "y", "a.b", "K" * 63):
            if probe and comps + (probe,) not in nodes:
                assert g.debug_json_schema_find(node, probe.encode("utf-8")) == (-1, -1)
    assert g.debug_json_schema_find(len(nodes) + 5, b"a") == (-1, -1)
