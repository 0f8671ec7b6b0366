"""JSON documents for the device JSON walker's tests (test_json_leaves_host.py: the walker on the host; test_gpu_json.py: the
kernels): one table of named edge documents with the status each must get, and seeded generators of documents that lie inside
the class the device must decide, of mutated ones and of random bytes.  No tests in here."""
import json

import numpy as np

OK, SYNTAX, DEPTH, PATH, KEY, DUP, TEXT = range(7)

SCHEMA = ["", "a", "a.b", "k", "items.index(0)", "items.index(2)", "m.n.o"]
SCHEMA_UTF8 = ["\u00e9", "\u65e5\u672c.\u8a9e", "K" * 62]

# what a walker that read past a document's end would complete its last token with
NEIGHBOUR = b'34e5"z"}]'


def deep_schema(n):
    return [".".join(["d"] * n)]


def deep_doc(n):
    return b'{"d":' * n + b'"x"' + b"}" * n


class Doc:
    def __init__(self, name, raw, status, schema=None, in_class=None):
        self.name, self.schema = name, SCHEMA if schema is None else schema
        self.raw = raw.encode("utf-8") if isinstance(raw, str) else bytes(raw)
        self.status = status                      # the status it must get
        # inside the class that MUST be decided on the device (status 0 guaranteed)
        self.in_class = (status == OK) if in_class is None else in_class

    def __repr__(self):
        return "Doc(%s)" % self.name


def _escape_run_docs():
    """a backslash run of 1, 2 and 3 in front of a quote, cut by the piece border after j of its backslashes"""
    out = []
    for r in (1, 2, 3):
        for j in range(0, r + 1):
            head = b'{"a":"'
            pad = 64 - j - len(head)
            tail = b'z"}' if r & 1 else b"}"
            out.append(Doc("backslash run %d, %d before the border" % (r, j), head + b"p" * pad + b"\\" * r + b'"' + tail, OK))
    return out


def _u_escape_docs():
    out = []
    for s in range(0, 7):
        head = b'{"a":"'
        out.append(Doc("\\u00e9 with %d bytes before the border" % s, head + b"p" * (64 - s - len(head)) + b'\\u00e9"}', OK))
    return out


def _sized(n):
    if n == 0:
        return Doc("0 bytes", b"", SYNTAX)
    if n == 1:
        return Doc("1 byte", b"7", OK)
    if n == 2:
        return Doc("2 bytes", b"[]", OK)
    return Doc("%d bytes" % n, b'"' + b"y" * (n - 2) + b'"', OK)


MALFORMED = ['{"a": }', '{"a" 1}', "[1, 2", '{"a": tru}', '{"a": "x\ny"}', '{"a": "\\q"}', "{} x", "", '{"a": 01}', '{"a": "\\u12G4"}',
             "[1,]", '{,}', '{"a": 1,}', "nul", "-", "1e", '"abc']
NO_LEAVES = ['{"a": 1, "b": [true, null, 2.5e3, {"c": {}}]}', "42", "[]", " {} ", "null", '{"a":{"a":{"a":[[[]]]}}}']


def table():
    t = []
    t += [Doc("malformed %r" % m, m, SYNTAX) for m in MALFORMED]
    t += [Doc("more malformed %r" % m, m, SYNTAX) for m in (
        "1.", "1.e3", "1e+", "-x", "+1", ".5", "00", "1 2", "tru e", "truefalse", "nulll", "[1 2]", '{"a":1 "k":2}', '{"a"}', "[}", "{]",
        '{"a":"x"', '["a",', "]", "}", ":", ",", '"\\', '"\\u00e', '"a\\u00e9', '{"a":"\\u00"}', "\x00", '"\x1f"', '"\t"', " ", "\n\t\r ",
        '{"a":1}}', "[[]", '"a" "b"', "1,", '\\"a"', '{"a":\\"x"}', "tRue", "0x10", "1e5.2", "--1", '{"a":"x",}', '[,1]', '{"a"::1}',
        "[" * 10001 + "]" * 10001)]
    t += [Doc("no leaves %r" % m, m, OK) for m in NO_LEAVES]
    t += [Doc("numbers", "[0, -0, 10, 1.5, -1.25e+10, 1E-2, 0e0, 0.0, 123456789012345678901234567890]", OK),
          Doc("whitespace", ' \n\t\r{ \n"a"\t:\r"x" ,\n"k" : "y" } \n', OK)]
    # piece borders
    t += [Doc("closing quote at byte %d" % (6 + n), '{"a":"' + "x" * n + '"}', OK) for n in (57, 58, 59)]
    t += _escape_run_docs()
    t += _u_escape_docs()
    t += [Doc("key ends at byte 63", "{" + " " * 61 + '"k":"v"}', OK),
          Doc("long key ends at byte 63", '{"' + "K" * 62 + '":"v"}', OK, SCHEMA_UTF8),
          Doc("number at the last byte", "12", OK), Doc("fraction at the last byte", "-1.5e3", OK),
          Doc("number at byte 63", "[" + " " * 61 + "12", SYNTAX), Doc("literal cut by the end", "[tru", SYNTAX),
          Doc("literal over the border", "[" + " " * 61 + "true, false ,null]", OK)]
    t += [_sized(n) for n in (0, 1, 2, 63, 64, 65, 127, 128)]
    # paths
    t += [Doc("top-level string", '"x"', OK), Doc("index(2) as a key", '{"items":{"index(2)":"x"}}', OK),
          Doc("array elements", '{"items":["p", 1, "q"]}', OK), Doc("key a.b with a string", '{"a.b":"x"}', PATH),
          Doc("key a.b with a number", '{"a.b":5}', OK), Doc("string at items.index(1)", '{"items":[1,"s"]}', PATH),
          Doc("unknown subtree without strings", '{"extra":[1,{"x":null}]}', OK), Doc("unknown subtree with a string", '{"extra":{"x":"s"}}', PATH),
          Doc("nested leaf", '{"a":{"b":"x"},"m":{"n":{"o":"y"}}}', OK), Doc("string at a prefix", '{"m":{"n":"y"}}', PATH),
          Doc("string under a leaf path", '{"k":{"z":"y"}}', PATH), Doc("top-level array of strings", '["x"]', PATH),
          Doc("eleven elements", '{"items":["p",1,"q",3,4,5,6,7,8,9,10,11]}', OK)]
    # duplicates
    t += [Doc("duplicate leaf key", '{"k":"first","k":"last"}', DUP), Doc("duplicate, second no string", '{"a":"x","a":5}', DUP),
          Doc("duplicate above a leaf", '{"a":{"b":"x"},"a":1}', DUP), Doc("duplicate prefix node", '{"m":1,"m":2}', DUP),
          Doc("duplicate under an unknown key", '{"zz":{"q":1,"q":2},"y":1,"y":2}', OK, in_class=False)]
    # depth
    t += [Doc("32 containers", deep_doc(32), OK, deep_schema(32)), Doc("33 containers", deep_doc(33), DEPTH, deep_schema(33)),
          Doc("32 arrays", "[" * 32 + "]" * 32, OK), Doc("33 arrays", "[" * 33 + "]" * 33, DEPTH),
          Doc("33 arrays, unclosed", "[" * 33 + "]" * 32, SYNTAX), Doc("100 mixed", '{"q":[' * 50 + "1" + "]}" * 50, DEPTH)]
    # keys
    t += [Doc("empty key", '{"":1}', KEY), Doc("escaped key", '{"a\\u0062":1}', KEY), Doc("invalid UTF-8 key", b'{"\xff":1}', KEY),
          Doc("escaped quote in a key", '{"a\\"b":1}', KEY), Doc("empty key deep in an unknown subtree", '{"zz":[{"":null}]}', KEY),
          Doc("non-ASCII keys", '{"\u00e9":"v","\u65e5\u672c":{"\u8a9e":"w"}}', OK, SCHEMA_UTF8),
          Doc("path before key", '{"a.b":"x","":1}', PATH)]
    # values
    t += [Doc("simple escapes", '{"a":"\\"\\\\\\/\\b\\f\\n\\r\\t"}', OK), Doc("\\u0000", '{"a":"x\\u0000y"}', OK),
          Doc("\\u00e9", '{"a":"\\u00e9\\u00E9"}', OK), Doc("\\u20ac", '{"a":"\\u20ac"}', OK), Doc("\\uffff", '{"a":"\\uffff\\ud7ff\\ue000"}', OK),
          Doc("raw UTF-8", '{"a":"\u00e9 \u20ac \U0001F600"}', OK), Doc("empty string", '{"a":"","k":""}', OK),
          Doc("70000 bytes", '{"a":"' + "lorem \\n ipsum \u20ac " * 3500 + '"}', OK),
          Doc("surrogate pair", '{"a":"\\ud83d\\ude00"}', TEXT), Doc("lone high surrogate", '{"a":"\\ud800"}', TEXT),
          Doc("lone low surrogate", '{"a":"\\udc00x"}', TEXT), Doc("invalid byte", b'{"a":"\xff"}', TEXT),
          Doc("overlong", b'{"a":"\xc0\x80"}', TEXT), Doc("cut sequence", b'{"a":"\xe2\x82"}', TEXT), Doc("lone continuation", b'{"a":"x\x80"}', TEXT),
          Doc("encoded surrogate", b'{"a":"\xed\xa0\x80"}', TEXT), Doc("above U+10FFFF", b'{"a":"\xf4\x90\x80\x80"}', TEXT),
          Doc("invalid byte at an unknown path", b'{"zz":"\xff"}', PATH), Doc("surrogate and bad path", '{"a":"\\ud800","zz":"s"}', PATH),
          Doc("UTF-8 over the border", '{"a":"' + "p" * 56 + '\u20ac\U0001F600"}', OK)]
    names = [d.name for d in t]
    assert len(set(names)) == len(names)
    return t


def at_alignment(doc, align):
    """the batch that puts doc at a byte offset of `align` (mod 64) in the blob, with a neighbour glued behind it: a filler document
    of `align` bytes in front (whitespace: not JSON)"""
    return [b" " * align, doc, NEIGHBOUR]


# ---- generators ---------------------------------------------------------------------------------------------------------
_ALPHABET = list("abcdefghij KLMNOP 0123456789 .,:{}[] ") + ['"', "\\", "/", "\n", "\t", "\r", "\b", "\f", "\x00", "\x1f", "\u00e9", "\u00df", "\u20ac",
                                                              "\u65e5", "\U0001F600", "\ufffd"]
_SIMPLE = {'"': '\\"', "\\": "\\\\", "\b": "\\b", "\f": "\\f", "\n": "\\n", "\r": "\\r", "\t": "\\t"}


def _string(s, rng):
    out = ['"']
    for ch in s:
        cp = ord(ch)
        if ch in _SIMPLE:
            out.append(_SIMPLE[ch])
        elif cp < 0x20:
            out.append("\\u%04x" % cp)
        elif ch == "/" and rng.random() < 0.5:
            out.append("\\/")
        elif cp < 0x10000 and not 0xD800 <= cp <= 0xDFFF and rng.random() < 0.15:
            out.append(("\\u%04x" if rng.random() < 0.5 else "\\u%04X") % cp)
        else:
            out.append(ch)
    out.append('"')
    return "".join(out)


def _ws(rng):
    return "" if rng.random() < 0.6 else "".join(" \n\t\r"[int(x)] for x in rng.integers(0, 4, int(rng.integers(1, 4))))


def dumps(v, rng):
    """v as JSON text: random whitespace between the tokens, random spellings of the escapes; keys are written raw"""
    if isinstance(v, Raw):
        return str(v)
    if isinstance(v, str):
        return _string(v, rng)
    if isinstance(v, dict):
        return "{" + ",".join(_ws(rng) + '"' + k + '"' + _ws(rng) + ":" + _ws(rng) + dumps(x, rng) + _ws(rng) for k, x in v.items()) + _ws(rng) + "}"
    if isinstance(v, list):
        return "[" + ",".join(_ws(rng) + dumps(x, rng) + _ws(rng) for x in v) + _ws(rng) + "]"
    return json.dumps(v)


class Raw(str):
    """a scalar given as its JSON text"""


_SCALARS = ["0", "-1", "3.25", "1e9", "-0.5E-3", "true", "false", "null", "12345678901234567890", "[]", "{}", "[1,[2,{}]]", '{"u":{"v":[null]}}']


def _scalar(rng):
    return Raw(_SCALARS[int(rng.integers(len(_SCALARS)))])


def _text(rng, words=None):
    if words and rng.random() < 0.7:
        t = " ".join(words[int(x)] for x in rng.integers(0, len(words), int(rng.integers(0, 6))))
        return t.upper() if rng.random() < 0.1 else t
    return "".join(_ALPHABET[int(x)] for x in rng.integers(0, len(_ALPHABET), int(rng.integers(0, 40))))


def gen_value(schema, rng, words=None, density=0.6):
    """a JSON-shaped Python value whose string leaves all lie at schema paths, with keys the schema does not know (holding no strings)
    mixed in -- inside the device class by construction.  Dicts keep their insertion order; list gaps hold scalars."""
    if "" in schema and rng.random() < 0.05:
        return _text(rng, words)
    root = {}
    for path in (schema[int(i)] for i in rng.permutation(len(schema))):
        comps = path.split(".")
        if path == "" or "" in comps or rng.random() > density:
            continue
        node = root
        for i, c in enumerate(comps):
            is_index = c.startswith("index(") and c.endswith(")") and c[6:-1].isdigit() and str(int(c[6:-1])) == c[6:-1]
            if node.setdefault(_KIND, is_index) != is_index:
                break                             # an object already (or an array): the path does not fit this document
            nxt = node.get(c)
            if i == len(comps) - 1:
                if nxt is None:
                    node[c] = _text(rng, words)
            elif nxt is None:
                nxt = node[c] = {}
            if not isinstance(nxt, dict):
                break
            node = nxt

    def finish(node):
        if not isinstance(node, dict):
            return node
        if node.pop(_KIND, False):
            size = max(int(k[6:-1]) for k in node) + 1 + int(rng.integers(0, 2))
            return [finish(node["index(%d)" % i]) if "index(%d)" % i in node else _scalar(rng) for i in range(size)]
        out = {}
        for k, v in node.items():
            if rng.random() < 0.3:
                out["x%d" % len(out)] = _scalar(rng)
            out[k] = finish(v)
        return out
    return finish(root)


_KIND = "\0kind"                                   # True: the container's children are array elements


def gen_doc(schema, rng, words=None, density=0.6):
    return dumps(gen_value(schema, rng, words, density), rng).encode("utf-8")


def mutate(raw, rng):
    """one random byte edit: a byte replaced, inserted or deleted"""
    raw = bytearray(raw)
    special = b'"\\{}[]:,u \n0-.e\x00\xff\x80\xc3t'
    b = special[int(rng.integers(len(special)))] if rng.random() < 0.7 else int(rng.integers(256))
    kind = int(rng.integers(3))
    at = int(rng.integers(len(raw) + 1))
    if kind == 0 and raw:
        raw[min(at, len(raw) - 1)] = b
    elif kind == 1 or not raw:
        raw.insert(at, b)
    else:
        del raw[min(at, len(raw) - 1)]
    return bytes(raw)


def random_bytes(rng):
    n = int(rng.integers(0, 200))
    if rng.random() < 0.5:
        return bytes(rng.integers(0, 256, n, dtype=np.uint8))
    pool = b'{}[]":,\\ abtrue0123.e-nfls\n'
    return bytes(pool[int(x)] for x in rng.integers(0, len(pool), n))


def corpus(schema, rng, n, words=None):
    """n documents: generated ones, and per generated one with probability 1/4 a mutated copy, 1/8 random bytes.  Returns
    (documents, flags: True where the document is an unmutated generated one)"""
    docs, clean = [], []
    while len(docs) < n:
        d = gen_doc(schema, rng, words)
        docs.append(d)
        clean.append(True)
        if rng.random() < 0.25:
            docs.append(mutate(d, rng))
            clean.append(False)
        if rng.random() < 0.125:
            docs.append(random_bytes(rng))
            clean.append(False)
    return docs[:n], clean[:n]


def leaves_of(status, rec_off, leaf_field, leaf_off, text):
    """the arrays of the record form -> one (status, [(field, bytes)]) per document"""
    out = []
    for d in range(len(status)):
        a, b = int(rec_off[d]), int(rec_off[d + 1])
        out.append((int(status[d]), [(int(leaf_field[l]), bytes(text[int(leaf_off[l]):int(leaf_off[l + 1])])) for l in range(a, b)]))
    return out


def to_device(docs):
    """documents -> (blob with 64 bytes of slack, doc_off) as device tensors"""
    import torch
    from gofindthem_amd.engine import pack
    blob, off = pack([d.encode("utf-8") if isinstance(d, str) else bytes(d) for d in docs])
    blob = np.concatenate([blob, np.zeros(64, dtype=np.uint8)])
    return torch.from_numpy(blob).cuda(), torch.from_numpy(off.astype(np.int64)).cuda()


def check_leaves(g, docs, caps=None):
    """JsonLeavesDevice == gft_debug_json_leaves_ref in every array; nothing stored behind the caps"""
    ref = g.debug_json_leaves_ref(docs, *(caps or ()))
    got = g.JsonLeavesDevice(*to_device(docs), *(caps or ()))
    n_leaves, n_text = ref[5]
    assert got[5] == ref[5]
    status, rec_off, leaf_field, leaf_off, text = (t.cpu().numpy() for t in got[:5])
    assert np.array_equal(status, ref[0]) and np.array_equal(rec_off.astype(np.uint64), ref[1])
    leaf_cap, text_cap = caps or ref[5]
    k, t = min(leaf_cap, n_leaves), min(text_cap, n_text)
    assert np.array_equal(leaf_field[:k].astype(np.uint32), ref[2][:k]) and np.all(leaf_field[leaf_cap:] == -1)
    end = k + 1 if n_leaves <= leaf_cap else k
    assert np.array_equal(leaf_off[:end].astype(np.uint64), ref[3][:end]) and np.all(leaf_off[max(leaf_cap + 1, end):] == -1)
    assert n_leaves <= leaf_cap or leaf_off[leaf_cap] == -1
    assert np.array_equal(text[:t], ref[4][:t]) and not text[text_cap:].any()
    return ref


def write_table(path):
    """the table as a data file for tools/json_walk_check.cpp: per document u32 paths, (u32 length, bytes) each, u32 status, u32
    length, the document"""
    import struct
    with open(path, "wb") as f:
        for d in table():
            f.write(struct.pack("<I", len(d.schema)))
            for p in d.schema:
                b = p.encode("utf-8")
                f.write(struct.pack("<I", len(b)) + b)
            f.write(struct.pack("<II", d.status, len(d.raw)) + d.raw)


if __name__ == "__main__":
    import sys
    write_table(sys.argv[1])
