"""Helpers of the tag result document tests (test_tags_json_host.py, test_gpu_tags_json.py): a restatement of the text format of
include/gft.h's gft_group_tags_json_device written from its description alone -- it builds dict[tag][path] = sorted(set(exprs))
from the leaf bitmap with plain Python, sorted by bytes, and joins the members, where the library permutes rows into slots,
counts costs and copies fragments --, seeded generators of expressions, schemas and batches, and a stats / assert_not_vacuous
pair.  No tests in here."""
import numpy as np

import rules_json as RJ
from gofindthem_amd import group
from gofindthem_amd.finder import EmptyRgxEngine, Finder, GpuEngine
from oracle import group_ref

GUARD = RJ.GUARD                 # what gofindthem_amd.group fills the text with before the call: behind the cap and inside holes
escape = RJ.escape               # dsl::json_str
assert_text = RJ.assert_text     # (text, out_off, total) against (text, out_off), under a cap
EMPTY_DOC = b'{"tags":{}}'
MAX_LEAVES = 1024                # GFT_TAGS_JSON_MAX_LEAVES
FRAGMENT_LENGTHS = (4, 5, 63, 64, 65, 255, 256, 257, 5000)
NASTY_TAGS = [b'q"uote', b"back\\slash", b"ctl\x01\x1f\n\r\t", "café 日本".encode("utf-8"), b"bad\xff\xc3utf8", b"del\x7f"]
NASTY_EXPRS = [b'"q\\"uote"', b'"back\\\\slash"', b'"ctl\x01\x1f\n\r\t"', '"café 日本"'.encode("utf-8"), b'"bad\xff\xc3utf8"', b'not "del\x7f"']
NASTY_PATHS = [b'p"q', b"p\\b", b"p\x01\x1f\n", "pé日".encode("utf-8"), b"p\xff\xc3", b"p\x7f"]
# the order of the text is unsigned bytes: "z" sorts in front of bytes >= 0x80; one string is a prefix of the other
ORDER_EXPRS = [b'"z"', b'"\xc3\xa9\xff"', b'"ab" or "c"', b'"ab"']


# ---- groups ----------------------------------------------------------------------------------------------------------------------
def finder_of(exprs, device=False):
    """a finder over [(expression bytes, tag bytes)]; device=False: one that needs no device"""
    f = Finder(GpuEngine(), EmptyRgxEngine(), False) if device else Finder(None, None, False, allow_no_device=True)
    for e, t in exprs:
        f.AddExpressionWithTag(e, t)
    return f


def group_of(exprs, schema, include=None, exclude=None, device=False):
    g = group.NewFinderWithRules(finder_of(exprs, device), {})
    g.SetSchema(schema, include, exclude)
    return g


def valid_fields(schema, include=None, exclude=None):
    """(the lists are ASCII; latin-1 keeps a path's bytes apart for the prefix tests)"""
    return [group_ref.is_valid_field_path(p.decode("latin-1"), include, exclude) for p in schema]


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def row_bits(row, E):
    bits = np.unpackbits(np.ascontiguousarray(row, dtype=np.uint32).view(np.uint8), bitorder="little")[:E]
    return [int(i) for i in np.flatnonzero(bits)]


def tag_map(exprs, schema, valid, leaves):
    """leaves: [(field index, [set expression indices])] -> {tag: {path: set(expression strings)}} of the valid fields"""
    m = {}
    for f, bits in leaves:
        if valid[f]:
            for e in bits:
                m.setdefault(exprs[e][1], {}).setdefault(schema[f], set()).add(exprs[e][0])
    return m


def document(m):
    tags = []
    for tag in sorted(m):
        fields = [escape(p) + b":[" + b",".join(escape(x) for x in sorted(m[tag][p])) + b"]" for p in sorted(m[tag])]
        tags.append(escape(tag) + b":{" + b",".join(fields) + b"}")
    return b'{"tags":{' + b",".join(tags) + b"}}"


def record_leaves(hits, E, field, rec_off, d):
    return [(int(field[l]), row_bits(hits[l], E)) for l in range(int(rec_off[d]), int(rec_off[d + 1]))]


def expected(exprs, schema, valid, hits, field, rec_off, hole_len=None):
    """-> (text bytes with GUARD in the holes, out_off u64[n + 1])"""
    E = len(exprs)
    hits = np.ascontiguousarray(hits, dtype=np.uint32).reshape(len(field), (E + 31) // 32)
    docs = []
    for d in range(len(rec_off) - 1):
        if hole_len is not None and int(hole_len[d]):
            docs.append(bytes([GUARD]) * int(hole_len[d]))
        else:
            docs.append(document(tag_map(exprs, schema, valid, record_leaves(hits, E, field, rec_off, d))))
    out_off = [1]
    for doc in docs:
        out_off.append(out_off[-1] + len(doc) + 1)
    return b"[" + b",".join(docs) + b"]", np.asarray(out_off, dtype=np.uint64)


def caps_for(want_text):
    """0, 1, 10, 11 (one short of the shortest document, and it), total - 1, total, and one in the middle of the first expression
    fragment of the text"""
    total = len(want_text)
    at = want_text.find(b'":["')
    mid = at + 6 if at >= 0 else total // 2             # (a fragment has at least 7 bytes and begins at at + 3)
    return [0, 1, 10, 11, max(total - 1, 0), total, min(mid, total)]


# ---- generators ------------------------------------------------------------------------------------------------------------------
def expr_of_fragment_length(n, fill=b"x"):
    """an expression whose fragment json_str(expr) has n bytes (n >= 7: the shortest expression is "x", its quotes escaped)"""
    assert n >= 7
    return b'"' + fill * (n - 6) + b'"'


def tag_of_fragment_length(n, head=b""):
    """a tag (or a path) whose fragment json_str(tag) + ':{' has n bytes (n >= 4)"""
    assert n >= 4 + len(head)
    return head + b"n" * (n - 4 - len(head))


def layout_exprs(slot_sizes, E=None, nasty=False, lengths=False):
    """[(expression, tag)] with slot_sizes[k] distinct expression strings under tag k.  Tag 0 is "" (TagText's).  Behind them:
    the first string of tag 0 once more under tag 0 (the two collapse into one slot), the same string under the last tag when it
    is another one (two slots: the sizes count it), then further repeats until there are E expressions.  Everything is registered
    in descending order of the expression string."""
    out = []
    for k, s in enumerate(slot_sizes):
        tag = b"" if k == 0 else b"t%03d" % k
        if nasty and k:
            tag += NASTY_TAGS[k % len(NASTY_TAGS)]
        if lengths and k:
            tag = tag_of_fragment_length(max(FRAGMENT_LENGTHS[k % len(FRAGMENT_LENGTHS)], 8), b"t%03d" % k)
        strings = list(ORDER_EXPRS) if k == 0 else []
        if k == len(slot_sizes) - 1 and k:
            strings.append(ORDER_EXPRS[0])                                    # the same string under two tags
        if nasty:
            strings += NASTY_EXPRS
        if lengths:
            strings += [expr_of_fragment_length(n, b"%d" % (k % 10)) for n in FRAGMENT_LENGTHS if n >= 7]
        strings = strings[:s]
        x = 0
        while len(strings) < s:
            strings.append(b'"k%d_%d"' % (k, x))
            x += 1
        out += [(e, tag) for e in strings]
    out.sort(key=lambda p: p[0], reverse=True)
    n = len(out)
    repeats = [out[-1 - (i % n)] for i in range(max((E or n + 1) - n, 0))]    # (from the lowest strings up: tag 0's "z" region)
    first0 = next(p for p in out if p[1] == b"")
    if repeats:
        repeats[0] = first0
    return out + repeats


def sizes_for_E(E):
    """slot sizes for a finder of E expressions: tags of 1, 2, 32, 33 and 70 slots as far as E has room, at least one repeat"""
    if E <= 2:
        return [1]
    sizes, left = [], E - 1
    for s in (33, 2, 1, 32, 70, 33, 7, 70, 33):
        if s <= left:
            sizes.append(s)
            left -= s
    if not sizes:
        sizes = [left]
    return sizes


def make_schema(F, reverse=True, nasty=False, lengths=False):
    """F unique paths, among them a / a.b / a0 and items.index(10) / items.index(2) (rank order is not index order), an excluded
    subtree "x" where F has room; reverse: listed in descending byte order"""
    paths = [b"a", b"a.b", b"a0", b"items.index(10)", b"items.index(2)", b"x", b"x.y"][:F]
    if nasty:
        paths += NASTY_PATHS
    if lengths:
        paths += [tag_of_fragment_length(n, b"L") for n in FRAGMENT_LENGTHS if n >= 5] + [b""]
    paths = paths[:F]
    k = 0
    while len(paths) < F:
        paths.append(b"f%d.g%d" % (k % 97, k))
        k += 1
    paths.sort(reverse=reverse)
    return paths


EXCLUDE = ["x"]                  # make_schema's excluded subtree


def slot_table(exprs):
    """{(tag, expression string): (tag's position, slot position inside the tag)} in output order"""
    by_tag = {}
    for e, t in exprs:
        by_tag.setdefault(t, set()).add(e)
    return {(t, e): (ti, si) for ti, t in enumerate(sorted(by_tag)) for si, e in enumerate(sorted(by_tag[t]))}


def make_batch(exprs, schema, valid, n_records, rng, leaves=None, density=0.15):
    """-> (hits u32[n_leaves, EW], field u32[n_leaves], rec_off u64[n_records + 1]): seeded records that name a field at most
    once, in random order, hit rows of mixed density with garbage bits at and above E; then -- where the shape has room -- the
    records that make a batch not vacuous planted over the first ones.  leaves: the leaf count of every record (default: 0 .. 6)"""
    E, F = len(exprs), len(schema)
    EW = (E + 31) // 32
    if leaves is None:
        leaves = [int(x) for x in rng.integers(0, min(F, 6) + 1, n_records)]
    recs = []                                                                   # [[(field, bit row u8[EW * 32])]]
    for L in leaves:
        fields = rng.permutation(F)[:L]
        dens = rng.choice([0.0, density, 0.6], p=[0.3, 0.5, 0.2])
        rec = []
        for f in fields:
            bits = np.zeros(EW * 32, dtype=np.uint8)
            bits[:E] = rng.random(E) < dens
            bits[E:] = rng.random(EW * 32 - E) < 0.5                          # garbage at and above E
            rec.append((int(f), bits))
        recs.append(rec)
    slots = slot_table(exprs)
    by_pair = {}
    for i, p in enumerate(exprs):
        by_pair.setdefault((p[1], p[0]), []).append(i)
    rank = {f: r for r, f in enumerate(sorted(range(F), key=lambda f: schema[f]))}
    good = sorted((f for f in range(F) if valid[f]), key=lambda f: rank[f])
    bad = [f for f in range(F) if not valid[f]]

    def row(on):
        bits = np.zeros(EW * 32, dtype=np.uint8)
        bits[list(on)] = 1
        return bits
    planted = [[]]                                                              # an empty record
    tags = sorted({t for _, t in exprs})
    shared = [v for v in by_pair.values() if len(v) >= 2]
    if good and E:
        two_of_a_tag = next(([i, j] for i in range(E) for j in range(i + 1, E) if exprs[i][1] == exprs[j][1] and exprs[i][0] != exprs[j][0]), None)
        other_tag = [next(i for i in range(E) if exprs[i][1] == t) for t in tags[:2]]
        on = set(other_tag) | set(two_of_a_tag or []) | set(shared[0] if shared else [])
        # two tags, two expressions of a field, a slot through two indices; two fields listed against their rank order
        planted.append([(f, row(on)) for f in reversed(good[:2])])
        late = [i for i, p in enumerate(exprs) if slots[(p[1], p[0])][1] >= 32]
        if late:
            planted.append([(good[-1], row([late[-1]]))])                      # a tag's only bit in the second word of its range
        if shared:
            planted.append([(good[0], row([shared[0][0]])), (good[-1], row([shared[0][-1]]))][:len(good)])
    if bad and E:
        planted.append([(bad[0], row(range(E)))] + ([(good[0], row([0]))] if good else []))   # a hit in an excluded field
    for k, rec in enumerate(planted[:n_records]):
        recs[k] = rec
    field = np.asarray([f for rec in recs for f, _ in rec], dtype=np.uint32)
    rec_off = np.cumsum([0] + [len(rec) for rec in recs]).astype(np.uint64)
    rows = [bits for rec in recs for _, bits in rec]
    hits = (np.packbits(np.asarray(rows, dtype=np.uint8).reshape(len(rows), EW * 32), axis=1, bitorder="little").view(np.uint32).reshape(len(rows), EW)
            if rows and EW else np.zeros((len(rows), EW), dtype=np.uint32))
    return hits, field, rec_off


def make_holes(n, rng, where="some"):
    """hole lengths u64[n]: first, last and two adjacent ones ("some"), or every record ("all")"""
    holes = np.zeros(n, dtype=np.uint64)
    if where == "all":
        holes[:] = rng.integers(11, 200, n)
        return holes
    for d in {0, n - 1, n // 2, n // 2 + 1}:
        if 0 <= d < n:
            holes[d] = int(rng.integers(11, 300))
    return holes


def stats(exprs, schema, valid, hits, field, rec_off, hole_len=None):
    E, F = len(exprs), len(schema)
    hits = np.ascontiguousarray(hits, dtype=np.uint32).reshape(len(field), (E + 31) // 32)
    slots = slot_table(exprs)
    rank = {f: r for r, f in enumerate(sorted(range(F), key=lambda f: schema[f]))}
    s = dict(two_tags=0, two_fields=0, two_exprs=0, shared_slot=0, out_of_rank=0, second_word=0, masked=0, empty=0, holes=0, garbage=0)
    for d in range(len(rec_off) - 1):
        if hole_len is not None and int(hole_len[d]):
            s["holes"] += 1
            continue
        leaves = record_leaves(hits, E, field, rec_off, d)
        m = tag_map(exprs, schema, valid, leaves)
        s["empty"] += not m
        s["two_tags"] += len(m) >= 2
        s["two_fields"] += any(len(fs) >= 2 for fs in m.values())
        s["two_exprs"] += any(len(v) >= 2 for fs in m.values() for v in fs.values())
        ranks = [rank[f] for f, bits in leaves if valid[f]]
        s["out_of_rank"] += ranks != sorted(ranks)
        for f, bits in leaves:
            s["masked"] += bool(bits) and not valid[f]
            pairs = [(exprs[e][1], exprs[e][0]) for e in bits]
            s["shared_slot"] += valid[f] and len(pairs) > len(set(pairs))
        for l in range(int(rec_off[d]), int(rec_off[d + 1])):
            s["garbage"] += len(row_bits(hits[l], hits.shape[1] * 32)) > len(row_bits(hits[l], E))
        for tag, fs in m.items():
            s["second_word"] += all(slots[(tag, x)][1] >= 32 for v in fs.values() for x in v)
    return s


def assert_not_vacuous(st, holes=False, tags=True, fields=True, exprs=True, shared=True, second_word=True, masked=True):
    """a generated batch holds a document with two tags, a tag with two fields, a field with two expressions, a slot reached
    through two expression indices, a record whose leaf order differs from rank order, a tag whose only set bits lie in the second
    word of its range, a hit in an excluded field, an empty document, and a hole where holes are used -- or the test fails.  The
    keyword arguments name what a shape cannot hold (one tag, one field, one expression, no repeat, no tag of more than 32 slots,
    nothing excluded), said by the caller"""
    assert st["empty"] > 0
    if tags:
        assert st["two_tags"] > 0
    if fields:
        assert st["two_fields"] > 0 and st["out_of_rank"] > 0
    if exprs:
        assert st["two_exprs"] > 0
    if shared:
        assert st["shared_slot"] > 0
    if second_word:
        assert st["second_word"] > 0
    if masked:
        assert st["masked"] > 0
    if holes:
        assert st["holes"] > 0
    return st


class Case:
    """one finder, schema and batch with the group, made once and left unchanged"""

    def __init__(self, exprs, schema, n_records, seed, exclude=EXCLUDE, leaves=None, density=0.15, device=False):
        self.exprs, self.schema, self.E = exprs, schema, len(exprs)
        self.g = group_of(exprs, schema, None, exclude, device)
        self.valid = valid_fields(schema, None, exclude)
        rng = np.random.default_rng([seed, len(exprs), len(schema), n_records])
        self.hits, self.field, self.rec_off = make_batch(exprs, schema, self.valid, n_records, rng, leaves, density)

    def want(self, holes=None):
        return expected(self.exprs, self.schema, self.valid, self.hits, self.field, self.rec_off, holes)

    def stats(self, holes=None):
        return stats(self.exprs, self.schema, self.valid, self.hits, self.field, self.rec_off, holes)

    def host(self, holes=None, cap=None):
        return self.g.debug_tags_json(self.hits, self.E, self.field, self.rec_off, holes, cap)

    def check(self, holes=None, cap=None):
        want = self.want(holes)
        assert_text(self.host(holes, cap), want, cap)
        return want
