"""fold_cases.py is what it claims (no GPU): the lists reach every piece byte, trip and wrong reading they were made for, the
restated rule is placement.fold_safe, the rule is what the product needs -- on a safe document the host's strings.ToLower
(gft_to_lower) is the ASCII fold, on a violation it is not, but for the kinds written out in CONSERVATIVE -- and the Python
unit slicing is unit_slice of gft_kernels.hpp as its comment states it."""
import numpy as np

import fold_cases as fc
import placement as pl
from tolower_cases import ref_lower

# kinds that the rule refuses although folding A-Z would do: a lower-case letter beyond Latin-1 (the long s) and a rune without
# case.  The rule looks at two bytes; it is allowed to be cautious, never to be lenient
CONSERVATIVE = ("C5 BF", "F0 9F 98 80")


def test_the_lists_hold_the_cases_they_were_made_for():
    log = {}
    fc.assert_not_vacuous(log)
    assert {r for r, _ in log} == set(fc.READINGS)
    for (reading, judge), case in sorted(log.items()):
        print("%-42s %-12s noticed by %s" % (reading, judge, case))
    bad, good = fc.n_single_cases()
    print("single-document cases: %d unsafe, %d safe" % (bad, good))


def test_the_restated_rule_is_the_walk():
    """rows_safe (no walk, whole arrays) against placement.fold_safe (the walk over one document) on every case of the shortest
    families, on the rim, and on random strings over the bytes the rule tells apart"""
    for key in [("unsafe", 40, f) for f in fc.FILLERS] + [("safe", 40, f) for f in fc.FILLERS] + [("rim", 0, f) for f in fc.FILLERS]:
        fam = fc.family(*key)
        for i, c in enumerate(fam.cases):
            assert pl.fold_safe(bytes(fam.doc(c.doc))) == (not fam.unsafe[i]), (fam.name, c)
    rng = np.random.default_rng(7)
    alphabet = np.frombuffer(bytes.fromhex("61 41 20 c2 c3 80 97 9e 9f a9 bf c4 e2 ff c0".replace(" ", "")), dtype=np.uint8)
    seen = set()
    for n in (1, 2, 3, 5, 8):
        rows = alphabet[rng.integers(0, len(alphabet), (3000, n))]
        got = fc.rows_safe(rows)
        for r, g in zip(rows, got):
            assert pl.fold_safe(bytes(r)) == bool(g), bytes(r).hex()
        seen |= set(got.tolist())
    assert seen == {True, False}
    assert fc.rows_safe(np.zeros((1, 0), np.uint8))[0] and fc.doc_safe(b"")


def test_the_rule_is_what_the_product_needs():
    """a case-insensitive finder folds A-Z and trusts the verdict for the rest: every safe document must lower-case to its ASCII
    fold, and every kind of violation must be one that folding gets wrong -- or stand in CONSERVATIVE"""
    n = 0
    for key in fc.SAFE_FAMILIES:
        fam = fc.family(*key)
        step = 1 if key[1] <= 1100 else 3 if key[1] < 8192 else 9          # (the long families: every ninth case and all kinds)
        for c in fam.cases[::step]:
            d = fam.doc(c.doc)
            assert ref_lower(d.tobytes()) == fc.ascii_fold(d), (fam.name, c)
            n += 1
        assert ref_lower(fam.doc(1).tobytes()) == fc.ascii_fold(fam.doc(1))            # (a spacer)
    assert n > 5000
    differs = {}
    for kind, v in fc.VIOLATIONS.items():
        for filler in fc.FILLERS:
            p = 39 if kind in fc.RIM_END else 0 if kind in fc.RIM_START else 17
            d = fc.build_doc(40, filler, p, v)
            assert not fc.doc_safe(d.tobytes())
            differs.setdefault(kind, set()).add(ref_lower(d.tobytes()) != fc.ascii_fold(d))
    for kind, s in differs.items():
        assert s == {kind not in CONSERVATIVE}, (kind, s)
    assert set(CONSERVATIVE) < set(fc.FREE)                                    # (nothing that the full sweeps are about)
    # upper-case text in the fillers: the fold has something to do
    assert any(65 <= b <= 90 for b in fc.build_doc(1000, "ascii", 0, b"\xc3\x89"))


def test_unit_slices_is_unit_slice():
    """gft_kernels.hpp: k = ceil(n / unit_max) units -- one up to unit_max bytes --, per = ceil(n / k) bytes each, the last one
    shorter; the units tile the document"""
    for n in fc.LENGTHS + (8191, 16384, 16385, 24576, 24577, 1, 0):
        u = fc.unit_slices(n)
        k = max(1, -(-n // fc.UNIT_MAX))
        per = -(-n // k)
        assert len(u) == k and u[0][0] == 0 and u[-1][1] == n
        assert all(a[1] == b[0] for a, b in zip(u, u[1:]))
        assert all(hi - lo == per for lo, hi in u[:-1]) and 0 <= u[-1][1] - u[-1][0] <= per <= fc.UNIT_MAX
    assert [len(fc.unit_slices(n)) for n in fc.LENGTHS] == [1] * 8 + [2, 3]
    assert fc.borders(20000)["unit 1"] == 6667 and fc.borders(8193)["unit 1"] == 4097 and "unit 1" not in fc.borders(8192)
    for n in fc.FULL:
        ps = set(fc.positions(n, 2, True))
        for b in fc.borders(n).values():
            assert set(range(max(b - 18, 0), min(b + 18, n - 1))) <= ps, (n, b)
        assert set(range(36)) <= ps and set(range(n - 37, n - 1)) <= ps
