"""Helpers of the rule result document tests (test_rules_json_host.py, test_gpu_rules_json.py): a restatement of the text format
of include/gft.h's gft_group_rules_json_device written from its description alone -- it builds every document as a list of
members and joins them, where the library counts costs and copies fragments --, seeded generators of rule sets and rule rows,
and the comparison of a result with the restatement.  No tests in here."""
import ctypes as C
import functools

import numpy as np

from gofindthem_amd import group
from gofindthem_amd.finder import Finder

GUARD = 0xA5                     # what gofindthem_amd.group fills the text with before the call: behind the cap and inside holes
EMPTY_DOC = b'{"rules":{}}'
FRAGMENT_LENGTHS = (4, 5, 63, 64, 65, 255, 256, 257, 5000)      # (2 and 3: see short_fragment_rules)


@functools.lru_cache(maxsize=None)
def escape(raw):
    """dsl::json_str: '"' and '\\' escaped, \\n \\r \\t, other bytes below 0x20 as \\u00xx in lower-case hex, every other byte raw
    (0x7F and bytes >= 0x80 included)"""
    out = bytearray(b'"')
    for c in bytes(raw):
        if c in (0x22, 0x5C):
            out += bytes([0x5C, c])
        elif c == 0x0A:
            out += b"\\n"
        elif c == 0x0D:
            out += b"\\r"
        elif c == 0x09:
            out += b"\\t"
        elif c < 0x20:
            out += b"\\u00" + b"0123456789abcdef"[c >> 4:(c >> 4) + 1] + b"0123456789abcdef"[c & 15:(c & 15) + 1]
        else:
            out.append(c)
    return bytes(out + b'"')


# ---- groups ----------------------------------------------------------------------------------------------------------------------
def add_rule_raw(g, name, expr):
    """AddRule with bytes: names and expressions that are not valid UTF-8 pass unchanged"""
    rc = g._L.gft_group_add_rule(g._h, bytes(name), len(name), bytes(expr), len(expr))
    if rc != 0:
        raise g._err(rc)


def raw_rule_exprs(g):
    """[(rule name, expression)] as bytes in the order of the rule bitmap's bits (gft_group_rule_expr)"""
    out = []
    name, expr, nl, el = C.c_void_p(), C.c_void_p(), C.c_uint32(), C.c_uint32()
    for i in range(g._L.gft_group_n_rule_exprs(g._h)):
        assert g._L.gft_group_rule_expr(g._h, i, C.byref(name), C.byref(nl), C.byref(expr), C.byref(el)) == 0
        out.append((C.string_at(name.value, nl.value) if nl.value else b"", C.string_at(expr.value, el.value) if el.value else b""))
    return out


def group_of(rules, finder=None):
    """a group over [(name bytes, [expression bytes])]; without a finder: one that needs no device"""
    g = group.GroupFinder(finder if finder is not None else Finder(None, None, False, allow_no_device=True))
    for name, exprs in rules:
        for e in exprs:
            add_rule_raw(g, name, e)
    return g


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def document(exprs, bits):
    """one document from the indices of its set bits (ascending)"""
    members = []                                  # [name, [expressions]] in bit order; a rule's bits are contiguous
    for i in bits:
        name, expr = exprs[i]
        if members and members[-1][2] == rule_start(exprs, i):
            members[-1][1].append(escape(expr))
        else:
            members.append([escape(name), [escape(expr)], rule_start(exprs, i)])
    return b'{"rules":{' + b",".join(n + b":[" + b",".join(es) + b"]" for n, es, _ in members) + b"}}"


_starts = {}


def rule_start(exprs, i):
    key = id(exprs)
    if key not in _starts or _starts[key][0] is not exprs:
        starts, s = [], 0
        for k in range(len(exprs)):
            if k and exprs[k][0] != exprs[k - 1][0]:
                s = k
            starts.append(s)
        _starts[key] = (exprs, starts)
    return _starts[key][1][i]


def row_bits(row, R):
    bits = np.unpackbits(np.ascontiguousarray(row, dtype=np.uint32).view(np.uint8), bitorder="little")[:R]
    return [int(i) for i in np.flatnonzero(bits)]


def expected(exprs, bitmap, hole_len=None):
    """-> (text bytes with GUARD in the holes, out_off u64[n + 1])"""
    R = len(exprs)
    bitmap = np.ascontiguousarray(bitmap, dtype=np.uint32).reshape(-1, (R + 31) // 32)
    docs = []
    for d in range(bitmap.shape[0]):
        if hole_len is not None and int(hole_len[d]):
            docs.append(bytes([GUARD]) * int(hole_len[d]))
        else:
            docs.append(document(exprs, row_bits(bitmap[d], R)))
    out_off = [1]
    for doc in docs:
        out_off.append(out_off[-1] + len(doc) + 1)
    return b"[" + b",".join(docs) + b"]", np.asarray(out_off, dtype=np.uint64)


def assert_text(got, want, cap=None):
    """got: (text with group.GroupFinder.TEXT_GUARD bytes behind the cap, out_off, total), numpy or torch; want: expected()'s"""
    text, out_off, total = got
    w_text, w_off = want
    text = np.asarray(text.cpu() if hasattr(text, "cpu") else text).astype(np.uint8)
    out_off = np.asarray(out_off.cpu() if hasattr(out_off, "cpu") else out_off).astype(np.uint64)
    assert total == len(w_text)
    assert np.array_equal(out_off, w_off)                                     # complete whatever the cap
    cap = total if cap is None else cap
    n = min(cap, total)
    assert len(text) > cap                                                     # (there are guard bytes to look at)
    assert bytes(text[:n]) == w_text[:n]                                       # hole bytes are GUARD on both sides
    assert (text[n:] == GUARD).all()                                           # nothing stored at or past the cap, nor behind it


def caps_for(exprs, bitmap, total):
    """0, 1, 11, 12, total - 1, total, and one in the middle of a fragment (the first expression fragment of the first document
    that has one)"""
    R = len(exprs)
    mid = total // 2
    at = 1
    bitmap = np.ascontiguousarray(bitmap, dtype=np.uint32).reshape(-1, (R + 31) // 32)
    for row in bitmap:
        bits = row_bits(row, R)
        if bits:
            head = at + len(b'{"rules":{') + len(escape(exprs[bits[0]][0])) + 2
            mid = head + max(1, len(escape(exprs[bits[0]][1])) // 2)
            break
        at += len(EMPTY_DOC) + 1
    return [0, 1, 11, 12, max(total - 1, 0), total, min(mid, total)]


# ---- generators ------------------------------------------------------------------------------------------------------------------
NASTY_NAMES = [b"", b'q"uote', b"back\\slash", b"ctl\x01\x1f\n\r\t", "café 日本".encode("utf-8"), b"bad\xff\xc3utf8", b"del\x7f"]
# (inside a tag the DSL reads \" and \\ as escapes; the expression string keeps them as written)
NASTY_EXPRS = [b'"q\\"uote"', b'"back\\\\slash"', b'"ctl\x01\x1f\n\r\t"', '"café 日本"'.encode("utf-8"), b'"bad\xff\xc3utf8"',
               b'not "del\x7f:f\\"p"']


def name_of_fragment_length(n, tag=b""):
    """a rule name whose fragment json_str(name) + ':[' has n bytes (n >= 4)"""
    assert n >= 4 + len(tag)
    return tag + b"n" * (n - 4 - len(tag))


def expr_of_fragment_length(n):
    """an expression whose fragment json_str(expr) has n bytes (n >= 7: the shortest expression is "x", its quotes escaped)"""
    assert n >= 7
    return b'"' + b"x" * (n - 6) + b'"'


def layout_rules(sizes, rng=None, nasty=False, lengths=False):
    """[(name, [expressions])] with sizes[k] expressions in rule k; names ascend bytewise in k, so rule k begins at bit
    sum(sizes[:k]).  nasty: the NASTY bytes inside names and expressions; lengths: fragments of FRAGMENT_LENGTHS"""
    rules = []
    x = 0
    for k, size in enumerate(sizes):
        name = b"r%04d" % k
        if nasty:
            name += NASTY_NAMES[k % len(NASTY_NAMES)]
        if lengths:
            name = name_of_fragment_length(max(FRAGMENT_LENGTHS[k % len(FRAGMENT_LENGTHS)], 9), b"r%04d" % k)
        exprs = []
        for _ in range(size):
            if lengths and x % 3 == 0:
                e = expr_of_fragment_length(max(FRAGMENT_LENGTHS[(x // 3) % len(FRAGMENT_LENGTHS)], 7))
            elif nasty and x % 2 == 0:
                e = NASTY_EXPRS[(x // 2) % len(NASTY_EXPRS)]
            else:
                e = b'"t%d"' % x if x % 5 else b'not "t%d:Field.%d"' % (x, x)
            exprs.append(e)
            x += 1
        rules.append((name, exprs))
    return rules


def short_fragment_rules():
    """name fragments of 4 and 5 bytes (the empty name and a one-byte name) in front of ordinary rules.  Fragments of 2 and 3
    bytes cannot come out of AddRule -- an expression has at least a quoted tag, 7 bytes escaped, a name fragment at least
    '"":[' -- and are covered by tools/rules_json_check.cpp, which hands make_rule_fragments arbitrary strings"""
    return [(b"", [b'"a"', b'"b"']), (b"a", [b'"a"']), (b"b", [b'"c"', b'"d"', b'"e"'])]


def sizes_for(R, rng):
    """rule sizes that sum to R: small rules, rules of more than 32 expressions, rules across word borders"""
    sizes = []
    left = R
    while left:
        s = int(rng.choice([1, 2, 3, 7, 33, 70])) if left > 8 else left
        s = min(s, left)
        sizes.append(s)
        left -= s
    return sizes


def sizes_with(size, begin, total=None):
    """a rule of `size` expressions that begins at bit `begin`, rules of 20, 11 and 1 in front of it as far as needed and a tail
    of small rules behind it"""
    front = {0: [], 20: [20], 31: [20, 11], 32: [20, 11, 1]}[begin]
    sizes = front + [size, 2, 1, 40]
    if total is not None and sum(sizes) < total:
        sizes.append(total - sum(sizes))
    return sizes


def make_rows(exprs, n_docs, rng, density=0.1):
    """n_docs rule rows u32[n_docs, RW]: seeded rows of mixed density, then -- where the shape has room -- the rows that make a
    batch not vacuous planted over the first ones: empty, all ones with garbage above R, two rules, two expressions of one rule, a
    straddling rule with bits on both sides of a word border, a rule whose only bit lies in a later word than its first bit"""
    R = len(exprs)
    RW = (R + 31) // 32
    bits = np.zeros((n_docs, RW * 32), dtype=np.uint8)
    if n_docs and R:
        dens = rng.choice([0.0, density, 0.5, 1.0], size=n_docs, p=[0.2, 0.5, 0.2, 0.1])
        bits[:, :R] = rng.random((n_docs, R)) < dens[:, None]
    planted = []
    starts = [rule_start(exprs, i) for i in range(R)]
    ends = {}
    for i, s in enumerate(starts):
        ends[s] = i + 1
    firsts = sorted(ends)
    if R:
        planted.append([])                                                    # an empty row
        planted.append(list(range(RW * 32)))                                  # every bit, garbage above R included
        if len(firsts) >= 2:
            planted.append([firsts[0], firsts[-1]])                           # two rules, one expression each
        two = [s for s in firsts if ends[s] - s >= 2]
        if two:
            planted.append([two[0], two[0] + 1])                              # two expressions of one rule
        for s in firsts:
            if (ends[s] - 1) // 32 > s // 32:                                 # the rule straddles a word border
                border = (s // 32 + 1) * 32
                planted.append([border - 1, border])                          # bits on both sides of it
                planted.append([ends[s] - 1])                                 # the only bit in a later word than the first bit
                break
    for k, row in enumerate(planted[:n_docs]):
        bits[k] = 0
        bits[k, row] = 1
    return np.packbits(bits, axis=1, bitorder="little").view(np.uint32).reshape(n_docs, RW)


def make_holes(n_docs, rng, where="some"):
    """hole lengths u64[n_docs]: first, last and two adjacent ones ("some"), or every document ("all")"""
    holes = np.zeros(n_docs, dtype=np.uint64)
    if where == "all":
        holes[:] = rng.integers(12, 200, n_docs)
        return holes
    for d in {0, n_docs - 1, n_docs // 2, n_docs // 2 + 1}:
        if 0 <= d < n_docs:
            holes[d] = int(rng.integers(12, 300))
    return holes


def stats(exprs, bitmap, hole_len=None):
    R = len(exprs)
    bitmap = np.ascontiguousarray(bitmap, dtype=np.uint32).reshape(-1, (R + 31) // 32)
    s = dict(empty=0, two_rules=0, two_exprs=0, straddle=0, later_word=0, holes=0, garbage=0)
    for d, row in enumerate(bitmap):
        if hole_len is not None and int(hole_len[d]):
            s["holes"] += 1
            continue
        bits = row_bits(row, R)
        all_bits = row_bits(row, bitmap.shape[1] * 32)
        s["garbage"] += len(all_bits) > len(bits)
        s["empty"] += not bits
        by_rule = {}
        for i in bits:
            by_rule.setdefault(rule_start(exprs, i), []).append(i)
        s["two_rules"] += len(by_rule) >= 2
        s["two_exprs"] += any(len(v) >= 2 for v in by_rule.values())
        for first, v in by_rule.items():
            words = {i // 32 for i in v}
            s["straddle"] += len(words) >= 2 and any(i % 32 == 31 and i + 1 in v for i in v)
            s["later_word"] += len(v) == 1 and v[0] // 32 > first // 32
    return s


def assert_not_vacuous(exprs, bitmap, hole_len=None, holes=False, straddle=True, rules=True):
    """a generated batch holds an empty row, a row with two rules true, a rule with two true expressions, a straddling rule with set
    bits on both sides of the border, a rule whose only set bit lies in a later word than its first bit, and a hole where holes
    are used -- or the test fails.  straddle=False / rules=False: shapes that cannot (every rule inside one word; a single rule or
    one expression a rule), said by the caller"""
    s = stats(exprs, bitmap, hole_len)
    assert s["empty"] > 0
    if rules:
        assert s["two_rules"] > 0 and s["two_exprs"] > 0
    if straddle:
        assert s["straddle"] > 0 and s["later_word"] > 0
    if holes:
        assert s["holes"] > 0
    return s
