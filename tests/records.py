"""Helpers of the record tests (test_records_host.py, test_gpu_records.py): seeded generators of schemas, finder expressions,
rules and record batches, and the expectation -- oracle/group_ref.py's evaluate_rules over the tag map that the reference's
walk would build for an object holding exactly a record's (path, string) leaves, with the CPU oracle as ProcessText.  No tests
in here."""
import numpy as np

from gofindthem_amd.workload import Workload
from oracle import group_ref
from oracle.pyoracle import Oracle, pack_strings

_W = None


def vocabulary(n=24):
    """n distinct lower-case words of Workload(300)'s dictionary, none inside another"""
    global _W
    if _W is None:
        _W = [t.decode("ascii") for t in Workload(300).terms() if 4 <= len(t) <= 9 and t.isalpha()]
    out = []
    for w in _W:
        if not any(w in o or o in w for o in out):
            out.append(w)
        if len(out) == n:
            return out
    raise AssertionError("vocabulary too small")


def make_schema(F):
    """F unique paths in groups of four: "G3", "G3.a", "G3.b.index(0)", "G30" -- "G3" is a byte prefix of all four and of the
    group G30..G39 as well, which is what strings.HasPrefix makes of it"""
    out = []
    g = 0
    while len(out) < F:
        out += ["G%d" % g, "G%d.a" % g, "G%d.b.index(0)" % g, "G%d0" % g]
        g += 1
        if g % 10 == 0:
            g += 1                       # ("G10" was listed as the fourth path of G1)
    out = list(dict.fromkeys(out))[:F]
    assert len(out) == F
    return out


def make_expressions(E, T, rng):
    """E finder expressions over the vocabulary and their tags (tag of expression i = "tag<i % T>")"""
    V = vocabulary()
    exprs = []
    for i in range(E):
        a, b = (V[int(x)] for x in rng.choice(len(V), 2, replace=False))
        k = i % 4
        exprs.append('"%s"' % a if k < 2 else '"%s" and "%s"' % (a, b) if k == 2 else 'inord("%s" and "%s")' % (a, b))
    return exprs, ["tag%d" % (i % T) for i in range(E)]


def make_rules(R, T, schema, rng, unknown_tags=True):
    """{name: [expression]} with R expressions in all: random and / or / not trees over "tag:prefix" units"""
    prefixes = [""] * 3 + schema[:8] + [p.split(".")[0] for p in schema[:12]] + ["G", "G0.a.nothing"]
    tags = ["tag%d" % t for t in range(T)] + (["nosuchtag"] if unknown_tags else [])

    def unit():
        t = tags[int(rng.integers(len(tags)))]
        p = prefixes[int(rng.integers(len(prefixes)))]
        return '"%s:%s"' % (t, p) if p else '"%s"' % t

    def tree(depth):
        r = rng.random()
        if depth >= 3 or r < 0.35:
            return unit() if rng.random() < 0.7 else "not " + unit()
        if r < 0.5:
            return "not (%s)" % tree(depth + 1)
        return "(%s) %s (%s)" % (tree(depth + 1), "and" if rng.random() < 0.5 else "or", tree(depth + 1))
    rules = {}
    for i in range(R):
        rules.setdefault("rule%02d" % int(rng.integers(max(1, R // 2))), []).append(tree(0))
    return rules


def make_records(N, schema, rng, max_leaves=4, words=5):
    """N records of 0..max_leaves (path, text) leaves; fields lean towards the front of the schema, texts are a few words of
    the vocabulary, now and then upper-case or empty"""
    V = vocabulary()
    recs = []
    for _ in range(N):
        rec = []
        for _ in range(int(rng.integers(0, max_leaves + 1))):
            f = min(int(rng.exponential(4.0)), len(schema) - 1) if rng.random() < 0.8 else int(rng.integers(len(schema)))
            text = " ".join(V[int(x)] for x in rng.integers(0, len(V), int(rng.integers(0, words + 1))))
            rec.append((schema[f], text.upper() if rng.random() < 0.15 else text))
        recs.append(rec)
    return recs


class Expectation:
    """the oracle side of one (finder expressions, rules, schema, include / exclude) configuration"""

    def __init__(self, exprs, tags, rules, schema, include=None, exclude=None, keywords=None, lower=None):
        self.exprs, self.tags, self.schema, self.include, self.exclude = exprs, tags, schema, include, exclude
        self.lower = lower               # non-ASCII batches: the reference's strings.ToLower, applied before the oracle's scan
        self.oracle = None
        if exprs:
            probe = Oracle([b"x"])
            kws, _ = probe.set_expressions(exprs, False)
            self.oracle = Oracle(sorted(k.encode("utf-8") if isinstance(k, str) else k for k in (keywords or kws)))
            self.oracle.set_expressions(exprs, False)
        self.ref = group_ref.GroupFinder(None)
        self.ref.add_rules(rules)
        # numbering of the rule bitmap: ascending rule name in byte order, AddRule order inside a name
        self.numbering = [(name, raw) for name in sorted(self.ref.rules, key=lambda s: s.encode("utf-8")) for raw, _ in self.ref.rules[name]]

    def hit_bitmap(self, texts):
        """the CPU oracle's ProcessText over every leaf: u32[n_leaves, ceil(E / 32)]"""
        words = (len(self.exprs) + 31) // 32
        if not texts or not self.exprs:
            return np.zeros((len(texts), words), dtype=np.uint32)
        raws = [t.encode("utf-8") if isinstance(t, str) else bytes(t) for t in texts]
        if self.lower is not None:
            raws = [self.lower(r) for r in raws]
        blob, off = pack_strings(raws)
        blob = np.concatenate([blob, np.zeros(64, dtype=np.uint8)])
        return self.oracle.process(blob, off, fold=self.lower is None)

    def rules_of(self, records, hits=None):
        """one expressionsByRule dict per record (group_ref.evaluate_rules of the record's tag map), and the tag maps"""
        if hits is None:
            hits = self.hit_bitmap([t for rec in records for _, t in rec])
        out, maps, l = [], [], 0
        for rec in records:
            tagmap = {}
            for path, _ in rec:
                if group_ref.is_valid_field_path(path, self.include, self.exclude):
                    for i in range(len(self.exprs)):
                        if int(hits[l, i >> 5]) >> (i & 31) & 1:
                            tagmap.setdefault(self.tags[i], {}).setdefault(path, set()).add(self.exprs[i])
                l += 1
            maps.append(tagmap)
            out.append(self.ref.evaluate_rules(tagmap))
        return out, maps

    def bitmap_of(self, rule_dicts):
        words = (len(self.numbering) + 31) // 32
        bm = np.zeros((len(rule_dicts), words), dtype=np.uint32)
        for r, d in enumerate(rule_dicts):
            for i, (name, raw) in enumerate(self.numbering):
                if raw in d.get(name, ()):
                    bm[r, i >> 5] |= np.uint32(1 << (i & 31))
        return bm

    def expected(self, records, hits=None):
        return self.bitmap_of(self.rules_of(records, hits)[0])

    def prefix_dependence(self, maps):
        """over (record, UNIT with a field path) where the record's tag map holds the UNIT's tag: (how many, how many of
        them only in fields outside the prefix -- the answers that the field masks alone decide)"""
        units = set()

        def collect(e):
            if e is None:
                return
            if e.Type == group_ref.UNIT_EXPR:
                if e.FieldPath:
                    units.add((e.Name, e.FieldPath))
                return
            collect(e.LExpr)
            collect(e.RExpr)
        for ws in self.ref.rules.values():
            for _, e in ws:
                collect(e)
        present = outside = 0
        for m in maps:
            for tag, prefix in units:
                if tag in m:
                    present += 1
                    outside += not any(fp.startswith(prefix) for fp in m[tag])
        return present, outside


def csr(records, schema):
    """records -> (texts, leaf_field u32[], rec_off u64[])"""
    index = {p: i for i, p in enumerate(schema)}
    texts = [t for rec in records for _, t in rec]
    field = np.asarray([index[p] for rec in records for p, _ in rec], dtype=np.uint32)
    rec_off = np.zeros(len(records) + 1, dtype=np.uint64)
    if records:
        rec_off[1:] = np.cumsum([len(rec) for rec in records], dtype=np.uint64)
    return texts, field, rec_off


def flatten(obj, path=""):
    """the (path, string) leaves of the reference's walk over a JSON-shaped value (group/finder/internal.go:9-97)"""
    if isinstance(obj, str):
        return [(path, obj)]
    if isinstance(obj, dict):
        if any(not isinstance(k, str) for k in obj):
            return []
        return [x for k, v in obj.items() for x in flatten(v, k if path == "" else path + "." + k)]
    if isinstance(obj, (list, tuple)):
        return [x for i, v in enumerate(obj) for x in flatten(v, ("index(%d)" % i) if path == "" else path + ".index(%d)" % i)]
    return []


A, B = vocabulary()[0], vocabulary()[1]


def named_rows():
    """(name, finder expressions, tags, rules, schema, include, exclude, records, expected rule dicts)"""
    e2 = ['"%s"' % A, '"%s"' % B]
    t2 = ["tag0", "tag1"]
    rows = []
    schema = ["Field3", "Field3.SomeField1", "Field30", "Field"]
    rules = {"r": ['"tag0:Field3"']}
    recs = [[(p, A)] for p in schema]
    rows.append(("prefix Field3 also matches Field30", e2, t2, rules, schema, None, None, recs, [{"r": ['"tag0:Field3"']}] * 3 + [{}]))
    rules = {"r": ['"tag0"']}
    recs = [[("Field3.SomeField1", A)], [("Field3", A)], [("Field", A)]]
    rows.append(("exclude beats include", e2, t2, rules, schema, ["Field3"], ["Field3.SomeField1"], recs, [{}, {"r": ['"tag0"']}, {}]))
    rules = {"r": ['"tag0"'], "s": ['"tag0:"']}
    recs = [[("Field30", A), ("Field", B)], [("Field", A)]]
    rows.append(("empty prefix, the tag only in an excluded field", e2, t2, rules, schema, None, ["Field30"], recs,
                 [{}, {"r": ['"tag0"'], "s": ['"tag0:"']}]))
    rules = {"r": ['"ghost"', 'not "ghost"', '"ghost:Field" or "tag1"']}
    recs = [[("Field", A)], [("Field", B)]]
    rows.append(("a tag the finder does not know", e2, t2, rules, schema, None, None, recs,
                 [{"r": ['not "ghost"']}, {"r": ['not "ghost"', '"ghost:Field" or "tag1"']}]))
    rules = {"r": ['"tag0"', '"tag0:x"']}
    rows.append(("field \"\": the TagText case", e2, t2, rules, [""], None, None, [[("", A)], [("", B)]], [{"r": ['"tag0"']}, {}]))
    rules = {"r": ['not "tag0"', '"tag0"']}
    rows.append(("a record without leaves", e2, t2, rules, schema, None, None, [[], [("Field", A)], []],
                 [{"r": ['not "tag0"']}, {"r": ['"tag0"']}, {"r": ['not "tag0"']}]))
    rules = {"r": ['not "tag0"', '"tag0" or "tag1"']}
    rows.append(("an empty-string leaf", e2, t2, rules, schema, None, None, [[("Field", "")], [("Field", ""), ("Field3", B)]],
                 [{"r": ['not "tag0"']}, {"r": ['not "tag0"', '"tag0" or "tag1"']}]))
    rules = {"r": ['"tag0:Field" and "tag1:Field"', '"tag0:Field3"']}
    rows.append(("one field listed twice", e2, t2, rules, schema, None, None, [[("Field", A), ("Field", B)], [("Field", B), ("Field", B)]],
                 [{"r": ['"tag0:Field" and "tag1:Field"']}, {}]))
    return rows
