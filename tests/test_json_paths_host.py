"""Path discovery without a device: gft_debug_emulate_json_paths runs the discovery mode of the walker that the kernels are
compiled from (csrc/gft_json_walk.hpp) on the host, 64-byte piece by piece, with the hash set and the pool as plain arrays (E);
gft_debug_json_paths_ref is the host route's JSON reader plus a walk that joins component lists (R), by code that shares nothing
with the walker.  For the documents the reader accepts the two give the same set; a document that is not JSON may add the paths
in front of its error to E.  The same batches drive k_json_paths in test_gpu_json_paths.py."""
import numpy as np
import pytest

import json_docs as J
import json_paths_cases as P
import records as R
from gofindthem_amd import _lib, finder, group

G = P.host_group()


def E(docs):
    return G.debug_emulate_json_paths(docs)


def Rf(docs):
    return G.debug_json_paths_ref(docs)


def both(docs, want):
    """E == R == want, nothing dropped"""
    paths, dropped, _ = E(docs)
    assert paths == Rf(docs) == P.as_bytes(want) and dropped == 0


def test_symbols_exist():
    L = _lib.load()
    for name in ("gft_group_json_paths_device", "gft_group_process_jsons_auto", "gft_group_json_auto_last", "gft_debug_emulate_json_paths",
                 "gft_debug_json_paths_ref"):
        assert hasattr(L, name) and name in _lib.SYMBOLS
    for name in ("JsonPathsDevice", "ProcessJsonsAuto", "json_auto_last", "debug_emulate_json_paths", "debug_json_paths_ref"):
        assert hasattr(group.GroupFinder, name)


TABLE = J.table()
_SCHEMA_GROUPS = {}


def accepted(doc):
    """the host route's reader takes the document (the status of the leaves reference is not SYNTAX)"""
    key = tuple(doc.schema)
    if key not in _SCHEMA_GROUPS:
        f = finder.Finder(None, None, False, allow_no_device=True)
        g = group.NewFinder(f)
        g.SetSchema(doc.schema)
        g._keep = f
        _SCHEMA_GROUPS[key] = g
    return int(_SCHEMA_GROUPS[key].debug_json_leaves_ref([doc.raw])[0][0]) != J.SYNTAX


@pytest.mark.parametrize("doc", TABLE, ids=[d.name[:40] for d in TABLE])
def test_table(doc):
    paths, dropped, hashes = E([doc.raw])
    ref = Rf([doc.raw])
    assert dropped == 0 and set(ref) <= set(paths) and paths == sorted(set(paths)) and len(hashes) >= len(paths)
    if accepted(doc):
        assert paths == ref
        if doc.status == J.OK:                        # every string value lies at a schema path, and each of those is found
            assert paths == sorted(P.flatten_paths(doc.raw)) and set(paths) <= set(P.as_bytes(doc.schema))
    else:
        assert ref == []


def test_table_as_one_batch():
    docs = [d.raw for d in TABLE]
    paths, dropped, _ = E(docs)
    assert dropped == 0 and set(Rf(docs)) <= set(paths)
    ok = [d.raw for d in TABLE if accepted(d)]
    assert E(ok)[0] == Rf(ok) and len(Rf(ok)) > 10


@pytest.mark.parametrize("seed,schema", [(1, J.SCHEMA), (2, R.make_schema(24)), (3, J.SCHEMA_UTF8 + J.SCHEMA)])
def test_generated_mutated_and_random_documents(seed, schema):
    rng = np.random.default_rng(seed)
    docs, clean = J.corpus(schema, rng, 350)
    paths, dropped, _ = E(docs)
    ref = Rf(docs)
    assert dropped == 0 and set(ref) <= set(paths)
    # document by document: equal where the reader accepts, nothing from the reference where it does not
    n_bad = 0
    for i, d in enumerate(docs):
        e, r = E([d])[0], Rf([d])
        if clean[i]:
            assert e == r == sorted(P.flatten_paths(d)), d
        else:
            assert set(r) <= set(e), d
            n_bad += e != r
    want = set().union(*(P.flatten_paths(d) for i, d in enumerate(docs) if clean[i]))
    assert want <= set(ref) and len(want) >= len(schema) - 2 and n_bad > 0


def test_root_string_and_nested_arrays():
    both([b'"x"'], [""])
    both([b' "x" ', b"5", b"[]"], [""])
    both([P.nested_arrays()], ["a.index(1).index(0).b", "a.index(1).index(1)", "a.index(2)"])
    both([b'["x",["y"]]'], ["index(0)", "index(1).index(0)"])
    both([b'{"items":{"index(2)":"x"}}', b'{"items":[1,2,"y"]}'], ["items.index(2)"])          # one path, one hash
    assert len(E([b'{"items":{"index(2)":"x"}}', b'{"items":[1,2,"y"]}'])[2]) == 1
    both([], [])
    both([b"{}", b"[1,2]", b'{"a":{"b":null}}'], [])


def test_depth_32_against_33():
    both([P.deep_doc(32)], [".".join(["d"] * 32)])
    both([P.deep_doc(33)], [])
    both([b"[" * 31 + b'"x"' + b"]" * 31], [".".join(["index(0)"] * 31)])
    both([b"[" * 32 + b'"x"' + b"]" * 32], [".".join(["index(0)"] * 32)])
    both([b"[" * 33 + b'"x"' + b"]" * 33], [])
    # back above the limit the stack is intact
    both([b'{"d":' * 32 + b'{"e":"deep"}' + b"}" * 31 + b',"up":"y"}'], ["up"])


def test_keys_that_give_no_path():
    both([b'{"":"x","a":"y"}'], ["a"])
    both([b'{"":{"b":"x","c":["y"]},"a":"y"}'], ["a"])
    both([b'{"a\\u0062":"x","q\\\\":{"z":"x"},"ok":"y"}'], ["ok"])
    both([b'{"\xff":"x","t":{"\xc3":["x"]},"ok":"y"}'], ["ok"])
    both([b'{"t":{"":"x","u":"v"}}'], ["t.u"])


def test_path_of_65535_bytes_against_65536():
    a, b = P.long_key(32767, 1), P.long_key(32767, 2)
    both([b'{"' + a + b'":{"' + b + b'":"x"}}'], [a + b"." + b])
    both([b'{"' + a + b'":{"' + b + b'q":"x"}}'], [])
    both([b'{"' + a + b'":{"' + b + b'q":"x","s":"y"}}'], [a + b".s"])
    k = P.long_key(65535, 3)
    both([b'{"' + k + b'":"x"}'], [k])
    both([b'{"' + k + b'q":"x","z":"y"}'], ["z"])
    both([b'{"' + k + b'q":{"in":"x"},"z":"y"}'], ["z"])


def test_a_key_with_a_dot_is_reported_as_one_component():
    """as csrc/gft_json_walk.hpp documents it: the path reads like that of the nested member; two hashes, one path"""
    both([b'{"a.b":"x"}'], ["a.b"])
    paths, dropped, hashes = E([b'{"a.b":"x"}', b'{"a":{"b":"y"}}'])
    assert paths == [b"a.b"] == Rf([b'{"a.b":"x"}', b'{"a":{"b":"y"}}']) and len(hashes) == 2 and dropped == 0


def test_the_hash_does_not_depend_on_where_the_piece_borders_fall():
    key = P.long_key(70, 7)
    doc = b'{"' + key + b'":{"inner":["x"]}}'
    want = E([doc])
    assert want[0] == [key + b".inner.index(0)"] and len(want[2]) == 1
    for align in range(64):
        assert E([b" " * align + doc]) == want
    assert E([b" " * a + doc for a in range(0, 64, 5)]) == want


def test_path_cap():
    doc = P.many_strings(P.PATH_CAP + 1)
    paths, dropped, hashes = E([doc])
    ref = Rf([doc])
    assert len(ref) == P.PATH_CAP + 1 and len(paths) == P.PATH_CAP and dropped >= 1 and len(hashes) == P.PATH_CAP + 1
    assert set(paths) <= set(ref)
    paths, dropped, _ = E([P.many_strings(P.PATH_CAP)])
    assert len(paths) == P.PATH_CAP and dropped == 0


def test_pool_overflow_from_few_long_paths():
    doc, want = P.pool_overflow_doc()
    fit = P.pool_fit(want)
    assert 100 < fit < len(want)
    paths, dropped, _ = E([doc])
    assert paths == sorted(want[:fit]) and dropped == len(want) - fit
    assert Rf([doc]) == sorted(want)


def test_refusals():
    L = _lib.load()
    blob = np.frombuffer(b"{}{}" + bytes(64), dtype=np.uint8)
    off = np.asarray([0, 4, 2], dtype=np.uint64)
    out, poff, n = np.zeros(64, dtype=np.uint8), np.zeros(9, dtype=np.uint64), np.zeros(1, dtype=np.uint64)
    u64p = lambda a: a.ctypes.data_as(_lib.C.POINTER(_lib.C.c_uint64))
    assert L.gft_debug_json_paths_ref(G._h, blob.ctypes.data, off.ctypes.data, 2, out.ctypes.data, 64, poff.ctypes.data, 8, None, u64p(n)) == _lib.GFT_E_INVALID
    assert L.gft_debug_emulate_json_paths(G._h, blob.ctypes.data, off.ctypes.data, 2, out.ctypes.data, 64, poff.ctypes.data, 8, None, u64p(n), None, None, 0,
                                          None) == _lib.GFT_E_INVALID
    # caps that are too small: GFT_E_INVALID and what is needed
    doc = np.frombuffer(b'{"abc":"x","de":"y"}' + bytes(64), dtype=np.uint8)
    off = np.asarray([0, 20], dtype=np.uint64)
    needed = np.zeros(2, dtype=np.uint64)
    for fn, tail in ((L.gft_debug_json_paths_ref, ()), (L.gft_debug_emulate_json_paths, (None, None, 0, None))):
        for caps in ((4, 8), (64, 1)):
            assert fn(G._h, doc.ctypes.data, off.ctypes.data, 1, out.ctypes.data, caps[0], poff.ctypes.data, caps[1], needed.ctypes.data, u64p(n),
                      *tail) == _lib.GFT_E_INVALID
            assert list(needed) == [5, 2] and n[0] == 2
        assert fn(G._h, doc.ctypes.data, off.ctypes.data, 1, out.ctypes.data, 5, poff.ctypes.data, 2, needed.ctypes.data, u64p(n), *tail) == 0
        assert bytes(out[:5]) == b"abcde" and list(poff[:3]) == [0, 3, 5]


def test_the_batches_of_the_gpu_file():
    """what test_gpu_json_paths.py expects of its batches holds on the host first"""
    docs, want = P.shared_paths_docs(200)
    both(docs, want)
    docs, want = P.key_length_docs()
    both(docs, want)
    deep = P.deep_then_shallow(300)
    paths, dropped, _ = E(deep)
    assert paths == Rf(deep) and dropped == 0 and 500 < len(paths) < 8000
    assert Rf(P.broken_docs()) == []
    both([P.many_strings(1000)], [b"items.index(%d)" % i for i in range(1000)])
