"""Batches for the tests of path discovery (test_json_paths_host.py: the walker's discovery mode on the host;
test_gpu_json_paths.py: k_json_paths and ProcessJsonsAuto).  The expected sets are computed at test time through
gft_debug_emulate_json_paths (E) and gft_debug_json_paths_ref (R).  No tests in here."""
import json

import numpy as np

import json_docs as J

PATH_CAP = 16384
POOL = 8 << 20


def host_group():
    """a group that needs no device: for the two debug calls"""
    from gofindthem_amd import finder, group
    f = finder.Finder(None, None, False, allow_no_device=True)
    g = group.NewFinder(f)
    g._keep = f
    return g


def deep_doc(n, leaf=b'"x"'):
    return b'{"d":' * n + leaf + b"}" * n


def nested_arrays():
    return b'{"a":[1,[{"b":"x"},"y"],"z"]}'          # a.index(1).index(0).b, a.index(1).index(1), a.index(2)


def many_strings(n, key="items"):
    """one document with an array of n strings: items.index(0) .. items.index(n - 1)"""
    return ('{"%s":[' % key + ",".join('"s"' for _ in range(n)) + "]}").encode()


def long_key(n, seed):
    """n key bytes, no '.', no backslash, different for every seed"""
    rng = np.random.default_rng(seed)
    return bytes(rng.choice(np.frombuffer(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789_-", dtype=np.uint8), n))


def pool_overflow_doc(n=150, k=30000):
    """n paths of 2 * k + 4 bytes or so under two keys of k bytes: more than the pool of 8 MiB holds, in one document of 60 KB"""
    a, b = long_key(k, 1), long_key(k, 2)
    inner = b",".join(b'"m%d":"x"' % i for i in range(n))
    return b'{"' + a + b'":{"' + b + b'":{' + inner + b"}}}", [a + b"." + b + b".m%d" % i for i in range(n)]


def pool_fit(paths):
    """how many of the paths, taken in this order, the pool holds (u32 length + bytes, padded to 4)"""
    at = 0
    for i, p in enumerate(paths):
        at += 4 + ((len(p) + 3) & ~3)
        if at > POOL:
            return i
    return len(paths)


def key_length_docs():
    """keys of 63, 64, 65 and 4 000 bytes at two depths"""
    docs, want = [], set()
    for n in (63, 64, 65, 4000):
        k1, k2 = long_key(n, n), long_key(n, n + 1)
        docs.append(b'{"' + k1 + b'":"v","top":{"' + k2 + b'":["w"]}}')
        want |= {k1, b"top." + k2 + b".index(0)"}
    return docs, sorted(want)


def shared_paths_docs(n):
    """n documents that share 8 paths"""
    rng = np.random.default_rng(5)
    docs = []
    for i in range(n):
        d = {"Title": "t%d" % i, "Body": "b", "Meta": {"Notes": "n", "Author": "a", "Tags": ["x", "y"]}, "items": [{"k": "v"}, int(rng.integers(9)), "s"]}
        docs.append(J.dumps(d, rng).encode())
    want = sorted(p.encode() for p in ("Title", "Body", "Meta.Notes", "Meta.Author", "Meta.Tags.index(0)", "Meta.Tags.index(1)", "items.index(0).k",
                                       "items.index(2)"))
    return docs, want


def deep_then_shallow(n):
    """documents with key stacks of 20 to 32 entries, arrays among them, in front of shallow ones whose keys differ: a stack entry
    that survived a document would show as a path that no document has"""
    docs = []
    for i in range(n):
        if i % 3 != 2:
            shape = i % 60                            # (60 shapes: some 2 000 distinct paths, far below the cap)
            rng = np.random.default_rng(shape)
            depth = int(rng.integers(20, 33))
            opens, closes = b"", b""
            for d in range(depth):
                if rng.random() < 0.3:
                    opens += b'[1,"e%d",' % d
                    closes = b"]" + closes
                else:
                    opens += b'{"deep%d_%d":' % (d, shape % 7)
                    closes = b',"after%d":"s"}' % d + closes
            docs.append(opens + b'"leaf"' + closes)
        else:
            docs.append(b'{"s%d":"v","t":["u",{"w%d":"x"}]}' % (i % 5, i % 4))
    return docs


def broken_docs():
    return [b"", b"{", b'{"a":', b"]", b"nul", b'{"a" "x"}', b"\xff\xfe", b"[1,,2]"]


def as_bytes(paths):
    return sorted(p.encode("utf-8") if isinstance(p, str) else bytes(p) for p in paths)


def flatten_paths(raw):
    """the paths of a document's string values as Python's json and the reference walk's flatten() give them"""
    import records as R
    return {p.encode("utf-8") for p, _ in R.flatten(json.loads(raw.decode("utf-8")))}
