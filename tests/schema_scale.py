"""Inputs at the size of a production schema for the group finder's device kernels (test_schema_scale_host.py: the host walker
and the host rule interpreter against their references; test_gpu_schema_scale.py: k_json, k_leaf_tags and k_record_rules):
JSON batches in which a wave walks many documents in a row, tries of thousands of nodes, keys of up to 65 535 bytes, array
indices of several digits; rule sets of up to 8 192 units, operand stacks of 32, 65 535 fields, records of hundreds of
leaves.  Every case is seeded and built once per process.  No tests in here."""
import functools
import re

import numpy as np

import json_docs as J
import records as R

ONE_CU = 0xFFFF                 # gft_set_cu_margin: a margin larger than the device leaves one CU, k_json then runs 8 blocks
WAVES_ONE_CU = 32               # ... of four waves


# ---- JSON ---------------------------------------------------------------------------------------------------------------
WIDE = ["p%d" % i for i in range(16383)]                            # 16 384 trie nodes with the root: the limit
NESTED = ["g%d.f%d" % (i, j) for i in range(60) for j in range(50)]  # 3 061 nodes
INDEX_AT = (0, 9, 10, 11, 99, 100, 101, 999, 1000)
INDICES = ["arr.index(%d)" % k for k in INDEX_AT] + ["index(1).index(10)"]
KEY_LENGTHS = (63, 64, 65, 127, 128, 129, 1000, 4097, 65535)


def _long_key(n):
    rng = np.random.default_rng([77, n])
    return bytes(rng.integers(ord("a"), ord("z"), n, dtype=np.uint8)).decode("ascii")      # ('z' is kept for the near misses)


LONG_KEY = {n: _long_key(n) for n in KEY_LENGTHS}
LONG_KEYS = [LONG_KEY[n] for n in KEY_LENGTHS] + ["n." + LONG_KEY[n] for n in KEY_LENGTHS]
SCHEMAS = {"default": J.SCHEMA, "wide": WIDE, "nested": NESTED, "long keys": LONG_KEYS, "indices": INDICES}


class JsonCase:
    """a batch over one of SCHEMAS.  clean: per document, True where the status must be 0 (None: not a mixed batch); want: the
    status of every document, where the case pins it; fields: the field of every leaf, where the case pins it"""

    def __init__(self, name, schema, docs, clean=None, want=None, fields=None):
        self.name, self.schema, self.clean, self.want, self.fields = name, schema, clean, want, fields
        self.docs = [d.encode("utf-8") if isinstance(d, str) else bytes(d) for d in docs]

    def __repr__(self):
        return "JsonCase(%s)" % self.name


@functools.lru_cache(None)
def corpus():
    """the 2 000 generated, mutated and random documents of test_gpu_json.py (J.corpus, seed 42)"""
    docs, clean = J.corpus(J.SCHEMA, np.random.default_rng(42), 2000)
    return JsonCase("corpus", "default", docs, clean)


@functools.lru_cache(None)
def default_table():
    docs = [d for d in J.table() if d.schema is J.SCHEMA]
    return JsonCase("table", "default", [d.raw for d in docs], want=[d.status for d in docs])


@functools.lru_cache(None)
def alignments():
    """test_gpu_json.py's alignment batch: every piece-border document at the 64 alignments, between a filler and a neighbour"""
    border = [d for d in J.table() if d.schema is J.SCHEMA and ("border" in d.name or "byte" in d.name)]
    docs, want = [], []
    for d in border:
        for align in range(64):
            docs += J.at_alignment(d.raw, align)
            want += [J.SYNTAX, d.status, J.SYNTAX]
    return JsonCase("alignments", "default", docs, want=want)


def tiled_count(n_cus):
    return 3 * 32 * n_cus + 37


@functools.lru_cache(None)
def tiled(n_cus):
    """at least three documents for each of the 32 * n_cus waves of the default grid: the corpus again and again, every tile in
    a random order of its own (the wave stride is a multiple of 32: a periodic layout would hand a wave one kind of document)"""
    base, n = corpus(), tiled_count(n_cus)
    rng = np.random.default_rng(43)
    order = np.concatenate([rng.permutation(len(base.docs)) for _ in range(n // len(base.docs) + 1)])[:n]
    return JsonCase("tiled over %d CUs" % n_cus, "default", [base.docs[i] for i in order], [base.clean[i] for i in order])


@functools.lru_cache(None)
def write_pass_order():
    """what makes the write pass skip a document, then what it walks: per wave of the 32, documents of status != 0, then documents
    without leaves, then clean ones, three times over"""
    table = J.table()
    bad = [d.raw for d in table if d.schema is J.SCHEMA and d.status != J.OK and len(d.raw) < 1000]
    bad += [b'{"a":{"a":{"a":[[["x', b'{"m":{"n":{"o":"x\x01y"}}}', b'{"m":{"n":{"q":[[1,2,{"q":"s"}]]}}}', b'{"a":{"b":"x"},"k":"y","k":"z"}']
    zero = [m.encode() for m in J.NO_LEAVES] + [b"[0, -0, 10, 1.5]", b'{"zz":{"q":[1,2,{"r":null}]}}']
    base = corpus()
    good = [d for d, c in zip(base.docs, base.clean) if c]
    docs, clean = [], []
    for k in range(3):
        docs += [bad[(64 * k + i) % len(bad)] for i in range(64)] + [zero[(64 * k + i) % len(zero)] for i in range(64)] + good[64 * k:64 * k + 64]
        clean += [False] * 64 + [True] * 128
    return JsonCase("write pass order", "default", docs, clean)


def _members(keys):
    return "{" + ",".join('"p%d":"v%d"' % (k, k) for k in keys) + "}"


@functools.lru_cache(None)
def wide_cover():
    """256 documents of 64 members: every key of the 16 383 is looked up once, in a random order"""
    perm = [int(k) for k in np.random.default_rng(44).permutation(len(WIDE))]
    docs = [_members(perm[d:d + 64]) for d in range(0, len(perm), 64)]
    want = [J.OK] * len(docs) + [J.DUP, J.PATH, J.DUP]
    docs += ['{"p16000":"a","p16000":"b"}', '{"p16383":"a"}', '{"p5":1,"p5":2}']
    return JsonCase("wide cover", "wide", docs, want=want, fields=perm)


@functools.lru_cache(None)
def strided_reset():
    """640 documents (20 per wave on one CU) that all hold "p16000" and a handful of other keys, each once -- a word of `visited`
    that a wave does not clear makes the next of them a duplicate --, and among them documents with a true duplicate"""
    rng = np.random.default_rng(45)
    docs, clean = [], []
    for _ in range(640):
        keys = [16000] + [int(k) for k in rng.choice(len(WIDE), int(rng.integers(3, 12)), replace=False) if k != 16000]
        keys = [keys[int(i)] for i in rng.permutation(len(keys))]
        dup = rng.random() < 0.15
        if dup:
            keys.insert(int(rng.integers(len(keys) + 1)), keys[int(rng.integers(len(keys)))])
        docs.append(_members(keys))
        clean.append(not dup)
    return JsonCase("strided reset", "wide", docs, clean)


def sparse_doc(schema, rng, words=None, share=0.02):
    """J.gen_doc over a random `share` of the schema's paths, all of them present"""
    some = [schema[int(i)] for i in rng.choice(len(schema), max(1, int(share * len(schema))), replace=False)]
    return J.gen_doc(some, rng, words, 1.0)


def mixed(schema, rng, n, words=None, p_mutated=0.5):
    """n documents: sparse_doc()s, and behind about every second of them a copy with two random byte edits"""
    docs, clean = [], []
    while len(docs) < n:
        d = sparse_doc(schema, rng, words)
        docs.append(d)
        clean.append(True)
        if rng.random() < p_mutated:
            docs.append(J.mutate(J.mutate(d, rng), rng))
            clean.append(False)
    return docs[:n], clean[:n]


@functools.lru_cache(None)
def nested():
    docs, clean = mixed(NESTED, np.random.default_rng(46), 300)
    return JsonCase("nested", "nested", docs, clean)


@functools.lru_cache(None)
def long_keys():
    """every key length at the top level and one level down, behind 0, 1, 37 and 63 spaces; per key its near misses of equal
    length (the last byte, byte 64, byte 0 differ) with a string (PATH) and with a number (OK, no leaves); one key of 65 536"""
    docs, want, fields = [], [], []
    for i, n in enumerate(KEY_LENGTHS):
        k = LONG_KEY[n]
        misses = [k[:-1] + "z", "z" + k[1:]] + ([k[:64] + "z" + k[65:]] if n > 64 else [])
        assert all(len(m) == n and m != k for m in misses)
        for pad in (0, 1, 37, 63):
            for down in (False, True):
                for key, value, status in [(k, '"v"', J.OK)] + [(m, v, s) for m in misses for v, s in (('"v"', J.PATH), ("7", J.OK))]:
                    body = '{"%s":%s}' % (key, value)
                    docs.append(" " * pad + ('{"n":%s}' % body if down else body))
                    want.append(status)
                    if key == k:
                        fields.append(i + len(KEY_LENGTHS) * down)
    docs += ['{"%s":"v"}' % ("q" * 65536), '{"n":{"%s":1}}' % ("q" * 65536)]
    want += [J.PATH, J.OK]
    return JsonCase("long keys", "long keys", docs, [s == J.OK for s in want], want, fields)


@functools.lru_cache(None)
def indices():
    def arr(n, strings):
        return '{"arr":[' + ",".join('"s%d"' % i if i in strings else str(i) for i in range(n)) + "]}"
    inner = ",".join(str(i) for i in range(10))
    docs = [arr(1001, INDEX_AT), arr(13, range(13)), '[0,[%s,"deep"]]' % inner, arr(1001, INDEX_AT + (98,)), arr(1002, INDEX_AT),
            arr(1002, INDEX_AT + (1001,)), ' [ 0 , [ %s , "deep" ] , 2 ] ' % inner, '[0,[%s,1,"deeper"]]' % inner, arr(101, (100, 10))]
    want = [J.OK, J.PATH, J.OK, J.PATH, J.OK, J.PATH, J.OK, J.PATH, J.OK]
    fields = list(range(9)) + [9] + list(range(9)) + [9] + [2, 5]
    return JsonCase("indices", "indices", docs, want=want, fields=fields)


# name -> the function that builds the case (on first use: collecting the tests builds nothing)
JSON_CASES = {"table": default_table, "alignments": alignments, "corpus": corpus, "tiled": lambda: tiled(256), "write pass order": write_pass_order,
              "wide cover": wide_cover, "strided reset": strided_reset, "nested": nested, "long keys": long_keys, "indices": indices}


def same_leaves(a, b):
    """two host results of the record form are equal in every array"""
    for x, y, what in zip(a[:5], b[:5], ("status", "rec_off", "leaf_field", "leaf_off", "text")):
        assert np.array_equal(x, y), what
    assert a[5] == b[5]


# ---- rules --------------------------------------------------------------------------------------------------------------
class RuleCase:
    """finder expressions, rules and a schema; records whose texts do not matter, with a leaf bitmap drawn from a seeded RNG in
    place of the scan; the oracle's rule rows of both, computed once"""

    def __init__(self, name, exprs, tags, rules, schema, records, hits, include=None, exclude=None):
        self.name, self.exprs, self.tags, self.rules, self.schema, self.records = name, exprs, tags, rules, schema, records
        self.include, self.exclude = include, exclude
        _, self.field, self.rec_off = R.csr(records, schema)
        self.hits = hits
        assert hits.shape == (len(self.field), (len(exprs) + 31) // 32) and hits.dtype == np.uint32
        self._want = None

    def __repr__(self):
        return "RuleCase(%s)" % self.name

    @property
    def exp(self):
        if self._want is None:
            self._exp = R.Expectation(self.exprs, self.tags, self.rules, self.schema, self.include, self.exclude)
            self._dicts, self._maps = self._exp.rules_of(self.records, self.hits)
            self._want = self._exp.bitmap_of(self._dicts)
        return self._exp

    @property
    def want(self):
        """R.Expectation.expected(records, hits)"""
        return self.exp and self._want

    @property
    def maps(self):
        return self.exp and self._maps

    def dirty_hits(self):
        """the bitmap with every bit at and above the number of expressions set in a row's last word"""
        dirty = self.hits.copy()
        if len(self.exprs) % 32:
            dirty[:, -1] |= np.uint32((0xFFFFFFFF << (len(self.exprs) % 32)) & 0xFFFFFFFF)
        return dirty

    def true_share(self, columns=None):
        """(true answers, all answers) over the rule expressions `columns` (default: all)"""
        n = len(self.exp.numbering)
        bits = np.unpackbits(self.want.view(np.uint8), axis=1, bitorder="little")[:, :n]
        if columns is not None:
            bits = bits[:, columns]
        return int(bits.sum()), int(bits.size)

    def high_unit_columns(self, floor=256):
        """the rule expressions whose units all have an index of at least `floor` in the compiled set: units are numbered by
        first use, in the order of the rule bitmap's bits"""
        order, columns = {}, []
        for i, (_, raw) in enumerate(self.exp.numbering):
            ids = [order.setdefault(u, len(order)) for u in re.findall(r'"([^"]*)"', raw)]
            if min(ids) >= floor:
                columns.append(i)
        return columns


def random_hits(n_leaves, E, density, rng):
    bits = rng.random((n_leaves, ((E + 31) // 32) * 32)) < density
    bits[:, E:] = False
    return np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little")).view(np.uint32).reshape(n_leaves, (E + 31) // 32)


def leaves(rng, schema, n, pick=None):
    """n leaves (path, "") with fields drawn uniformly, or by pick()"""
    return [(schema[int(pick()) if pick else int(rng.integers(len(schema)))], "") for _ in range(n)]


def trees(units, n, rng, depth_max=3):
    """n random and / or / not trees over the UNIT strings `units` (the shape of R.make_rules)"""
    def unit():
        return '"%s"' % units[int(rng.integers(len(units)))]

    def tree(depth):
        r = rng.random()
        if depth >= depth_max or r < 0.35:
            return unit() if rng.random() < 0.7 else "not " + unit()
        if r < 0.5:
            return "not (%s)" % tree(depth + 1)
        return "(%s) %s (%s)" % (tree(depth + 1), "and" if rng.random() < 0.5 else "or", tree(depth + 1))
    return [tree(0) for _ in range(n)]


def nested_rule(units, depth, rng):
    """a right-nested chain over random units, "or" and "and not" mixed, whose postfix program needs an operand stack of exactly
    `depth`"""
    pick = lambda: '"%s"' % units[int(rng.integers(len(units)))]
    s = pick()
    for _ in range(depth - 1):
        s = ("%s or (%s)" if rng.random() < 0.5 else "%s and not (%s)") % (pick(), s)
    return s


UNIT_FIELDS = ["f%d" % i for i in range(128)]
UNIT_COUNTS = (255, 256, 257, 300, 8192)
UNIT_SEEDS = {257: 2}                # (where seed 0 does not meet the conditions that test_schema_scale_host.py sets)


def _unit_records(rng):
    sizes = [0, 40] + [int(x) for x in rng.integers(0, 41, 126)] + [257, 600]
    order = rng.permutation(len(sizes))
    return [leaves(rng, UNIT_FIELDS, sizes[int(i)]) for i in order]


@functools.lru_cache(None)
def unit_case(n_units, deep=0):
    """n_units distinct "tag<t>:f<i>" units of the 64 x 128, shuffled into OR-chains of 8 under one rule name -- unit k of the
    compiled set is the k-th of the shuffle --; deep: as many right-nested rules of stack depth 32 over random units behind them"""
    rng = np.random.default_rng([50, n_units, deep, UNIT_SEEDS.get(n_units, 0)])
    exprs, tags = ['"%s"' % R.A] * 64, ["tag%d" % t for t in range(64)]
    units = ["tag%d:f%d" % (t, i) for t in range(64) for i in range(128)]
    units = [units[int(i)] for i in rng.permutation(len(units))[:n_units]]
    rules = {"r": [" or ".join('"%s"' % u for u in units[k:k + 8]) for k in range(0, n_units, 8)]}
    if deep:
        rules["z_deep"] = [nested_rule(units, 32, rng) for _ in range(deep)]
    records = _unit_records(rng)
    hits = random_hits(sum(len(r) for r in records), 64, 0.5, rng)
    return RuleCase("%d units%s" % (n_units, ", %d rules of depth 32" % deep if deep else ""), exprs, tags, rules, UNIT_FIELDS, records, hits)


@functools.lru_cache(None)
def depth_case(depth):
    """a small set whose deepest operand stack is exactly `depth`"""
    rng = np.random.default_rng([51, depth])
    schema = R.make_schema(8)
    exprs, tags = R.make_expressions(40, 5, rng)
    units = ["tag%d:%s" % (t, p) for t in range(5) for p in ("G0", "G0.a", "G1", "G", "G10", "G2.b")]
    rules = {"deep": [nested_rule(units, depth, rng) for _ in range(6)], "flat": trees(units, 6, rng)}
    records = [leaves(rng, schema, int(rng.integers(0, 5))) for _ in range(130)]
    hits = random_hits(sum(len(r) for r in records), 40, 0.04, rng)
    return RuleCase("depth %d" % depth, exprs, tags, rules, schema, records, hits)


BIG_F = ["s%d.t%d" % (i >> 8, i & 255) for i in range(65535)]     # field 256 a + b is "s<a>.t<b>"; "s255.t31" is bit 31 of word 2040
BIG_F_PREFIXES = ("s255", "s25", "s2", "s255.t31", "s255.t32", "s0", "s0.t1")
BIG_F_FIELDS = (0, 1, 255, 256, 65534, 65311, 65312, 65279, 65280, 6399, 6400, 6655, 6656, 63999, 64000, 511, 512, 767, 768, 5119, 5120, 7679,
                7680, 51199, 51200, 31, 32, 2047, 2048)


@functools.lru_cache(None)
def field_words_case():
    """65 535 fields, 2 048 mask words: prefixes whose field ranges cross word borders, leaves on both sides of them"""
    rng = np.random.default_rng(52)
    exprs, tags = R.make_expressions(40, 5, rng)
    units = ["tag%d:%s" % (t, p) for t in range(5) for p in BIG_F_PREFIXES] + ["tag%d" % t for t in range(5)]
    rules = {"rule%02d" % (i // 3): [] for i in range(24)}
    for i, t in enumerate(trees(units, 24, rng)):
        rules["rule%02d" % (i // 3)].append(t)
    pick = lambda: BIG_F_FIELDS[int(rng.integers(len(BIG_F_FIELDS)))] if rng.random() < 0.8 else rng.integers(len(BIG_F))
    records = [leaves(rng, BIG_F, int(rng.integers(0, 6)), pick) for _ in range(130)]
    records[7] = [(BIG_F[f], "") for f in BIG_F_FIELDS]
    hits = random_hits(sum(len(r) for r in records), 40, 0.06, rng)
    return RuleCase("65535 fields", exprs, tags, rules, BIG_F, records, hits)


@functools.lru_cache(None)
def include_exclude_case():
    """1 000 fields under include and exclude lists"""
    rng = np.random.default_rng(53)
    schema = R.make_schema(1000)
    exprs, tags = R.make_expressions(40, 5, rng)
    units = ["tag%d:%s" % (t, p) for t in range(5) for p in ("G1", "G10", "G2", "G25", "G250.a", "G1.b", "G")] + ["tag%d" % t for t in range(5)]
    rules = {"r": trees(units, 24, rng)}
    near = [i for i, p in enumerate(schema) if p.startswith("G1") or p.startswith("G2")]
    pick = lambda: near[int(rng.integers(len(near)))] if rng.random() < 0.7 else rng.integers(len(schema))
    records = [leaves(rng, schema, int(rng.integers(0, 6)), pick) for _ in range(130)]
    hits = random_hits(sum(len(r) for r in records), 40, 0.06, rng)
    return RuleCase("1000 fields, include and exclude", exprs, tags, rules, schema, records, hits, include=["G1", "G2", "G30"], exclude=["G1.b", "G25"])


@functools.lru_cache(None)
def four_words_case():
    """100 expressions under 97 tags: four words of expressions, four of tags"""
    rng = np.random.default_rng(54)
    schema = R.make_schema(8)
    exprs, tags = R.make_expressions(100, 97, rng)
    rules = R.make_rules(33, 97, schema, rng)
    records = R.make_records(130, schema, rng, max_leaves=8)
    hits = random_hits(sum(len(r) for r in records), 100, 0.3, rng)
    return RuleCase("100 expressions, 97 tags", exprs, tags, rules, schema, records, hits)


@functools.lru_cache(None)
def chunks_case():
    """blocks of 64 records: 64 of 300 leaves (75 chunks of 256); one whose only tagged leaf is the last leaf of its last chunk;
    one with records of exactly 256 and 257 leaves and an empty record between two of 300"""
    rng = np.random.default_rng(55)
    schema = R.make_schema(8)
    exprs, tags = R.make_expressions(40, 5, rng)
    rules = R.make_rules(12, 5, schema, rng)
    sizes = [300] * 64 + [5] * 64 + [256, 257, 300, 0, 300] + [int(x) for x in rng.integers(0, 4, 20)]
    records = [leaves(rng, schema, n) for n in sizes]
    hits = random_hits(sum(sizes), 40, 0.002, rng)
    a, b = 64 * 300, 64 * 300 + 64 * 5
    hits[a:b] = 0
    hits[b - 1] = random_hits(1, 40, 1.0, rng)[0]
    return RuleCase("leaf chunks", exprs, tags, rules, schema, records, hits)


RULE_CASES = {"%d units" % n: functools.partial(unit_case, n) for n in UNIT_COUNTS}
RULE_CASES.update({"8192 units, depth 32": functools.partial(unit_case, 8192, 8), "depth 31": functools.partial(depth_case, 31),
                   "depth 32": functools.partial(depth_case, 32), "65535 fields": field_words_case, "1000 fields": include_exclude_case,
                   "four words": four_words_case, "leaf chunks": chunks_case})


# ---- end to end ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def end_to_end():
    """(finder expressions, tags, rules, 300 generated documents over NESTED, the batch they come from with a mutated copy behind
    about every second of them, its flags)"""
    rng = np.random.default_rng(56)
    exprs, tags = R.make_expressions(40, 5, rng)
    rules = R.make_rules(20, 5, NESTED, rng)
    V = R.vocabulary()
    broken, clean = mixed(NESTED, rng, 450, V)
    docs = [d for d, c in zip(broken, clean) if c][:300]
    return exprs, tags, rules, docs, broken, clean
