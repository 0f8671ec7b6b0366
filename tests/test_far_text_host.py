"""far_text.py is what it claims (no GPU): the filler depends on the high bits of its position, its torch form is its numpy form,
and it spells no keyword; the long batch's layout puts both crossings of 2^32 inside island 4; the sparse references, at a
scaled-down size, are the dense references of the case modules over the whole batch; and the comparison the GPU test uses notices
every mutant of the kinds a 32-bit slip gives."""
import numpy as np
import pytest

import far_text as F
import placement as pl

B = F.B
WINDOWS = [0, 1 << 20, (1 << 21) - 512, (1 << 26) - 512, B - (1 << 16), B - 512, B, B + (1 << 21), (1 << 32) + (1 << 30) + 12345, 4 * (1 << 30) + (600 << 20)]
PERIODS = (1 << 21, 1 << 26, 1 << 32)
KEYWORDS = F.TERMS + [F.HIT, F.OPEN, F.CLOSE, bytes([F.MASK])] + [r for r in F.REPS if r]


def test_filler_is_not_periodic_where_the_old_ramp_was():
    for w in WINDOWS:
        a = F.filler_range(w, w + 1024)
        raw = F.top_byte(np.arange(w, w + 1024, dtype=np.int64))
        for p in PERIODS:
            assert not np.array_equal(a, F.filler_range(w + p, w + p + 1024)), (w, p)
            assert not np.array_equal(raw, F.top_byte(np.arange(w + p, w + p + 1024, dtype=np.int64))), (w, p)
        # pointwise: 2^32 and 64 MiB further on the raw top byte, and 2^32 further on the filler itself, never hold the same
        assert (raw != F.top_byte(np.arange(w + B, w + B + 1024, dtype=np.int64))).all(), w
        assert (raw != F.top_byte(np.arange(w + (1 << 26), w + (1 << 26) + 1024, dtype=np.int64))).all(), w
        assert (a != F.filler_range(w + B, w + B + 1024)).all(), w
    # the ramp this replaces repeats every 2 MiB
    old = lambda p: ((p * 2654435761) >> 13) & 0xFF               # noqa: E731
    p = np.arange(5000, 6024, dtype=np.int64)
    assert all(np.array_equal(old(p), old(p + q)) for q in PERIODS)


def test_the_torch_form_is_the_numpy_form():
    torch = pytest.importorskip("torch")
    table = torch.frombuffer(bytearray(F.ALPHABET), dtype=torch.uint8)
    for w in WINDOWS:
        pos = torch.arange(w, w + 4096, dtype=torch.int64)
        assert np.array_equal(F.filler_torch(pos, table).numpy(), F.filler_range(w, w + 4096)), w
        assert np.array_equal(F.top_byte_torch(pos).to(torch.uint8).numpy(), F.top_byte(np.arange(w, w + 4096, dtype=np.int64))), w


def test_the_filler_spells_no_keyword():
    letters = set(b"".join(KEYWORDS))
    assert not letters & set(F.ALPHABET) and all(k for k in KEYWORDS)
    assert b"\n" not in F.ALPHABET and max(F.ALPHABET) < 0x80 and not any(65 <= b <= 90 for b in F.ALPHABET)
    sample = b"".join(F.filler_range(w, w + (1 << 17)).tobytes() for w in WINDOWS[:8])
    assert len(sample) == 1 << 20
    assert not any(k in sample for k in KEYWORDS)
    assert len(set(sample)) == 32                                   # every letter of the alphabet occurs


def test_border_placements():
    for size in (1, 40, 8292, F.WINDOW - 1):
        ps = dict(F.border_placements(size))
        assert list(ps) == list(F.BORDER_NAMES)
        assert ps["B-size"] + size == B and ps["B-size-1"] + size + 1 == B < ps["B-size-1"] + size + F.SLACK
        assert all(0 <= at and at + size + F.SLACK <= B + F.WINDOW + F.SLACK for at in ps.values())
        assert {0, 1, 15} <= {at % 16 for at in ps.values()}
    assert F.fits(F.WINDOW - 1) and not F.fits(F.WINDOW)
    assert F.strictly_inside(B - 17, [(0, 4), (16, 18)]) and not F.strictly_inside(B - 17, [(0, 17), (17, 30)])


def test_the_layout_of_the_long_batch():
    lb = F.long_batch()
    assert [lb.docs[i].body is None for i in lb.long_at] == [True] * 5 and len(lb.long_at) == 5
    assert all(lb.docs[i].length < 1 << 30 for i in lb.long_at) and all(lb.docs[i].length > (1 << 30) - (1 << 20) for i in lb.long_at[:4])
    assert 4.5 * (1 << 30) < lb.total < 4.7 * (1 << 30)
    d4 = lb.island_at[4]
    doc = lb.docs[d4]
    assert doc.length >= 8192 and lb.off[d4] < B < lb.off[d4 + 1] and lb.cross == B
    inside = B - lb.off[d4]
    assert 2048 < inside < doc.length - 2048                        # the middle of island 4 ...
    assert any(a < inside < a + n for a, n, _ in doc.spans), "no span of island 4 covers position 2^32"
    assert lb.off[lb.long_at[4]] > B                                # long_4 and island 5 lie wholly past it
    for i in lb.long_at:                                            # hits near both ends: in-document positions near 2^30
        starts = [a for a, n, _ in lb.docs[i].spans]
        assert min(starts) < 64 and max(starts) + len(F.HIT) > lb.docs[i].length - 64
        assert any((lb.off[i] + a) // F.TILE != (lb.off[i] + a + n - 1) // F.TILE for a, n, _ in lb.docs[i].spans if n)
        assert any(a // F.TILE != (a + n - 1) // F.TILE for a, n, _ in lb.docs[i].spans if n)
    for call in F.GROWING:
        at_in, at_out, delta = F.crossings(call)
        print("%s: input position 2^32 is byte %d of island 4; the island begins at output position 2^32 %+d; net change in front %+d"
              % (call, inside, at_out - B, delta))
        assert abs(delta) < 2048, "%s: the net length change in front of island 4 is %d" % (call, delta)
        w = F.sparse(call)
        assert w["out_off"][d4] < B < w["out_off"][d4 + 1], "%s: the output's crossing of 2^32 lies outside island 4" % call


TWIN = 3 * F.TILE + 37


@pytest.mark.parametrize("call", sorted(F.SPARSE))
def test_sparse_references_are_the_dense_ones_on_the_scaled_down_batch(call):
    lb = F.long_batch(TWIN)
    assert all(lb.docs[i].length >= 3 * F.TILE for i in lb.long_at)
    text = lb.dense()
    assert all(text[p:p + len(h)] == h for i in lb.long_at for p, h in lb.hits(i))
    w, dense = F.sparse(call, TWIN), F.dense_reference(call, lb)
    assert F.materialise(w["segs"], text) == dense["out"], call
    for k, v in w.items():
        if k != "segs":
            assert v == dense[k], (call, k)
    assert set(dense) - {"out"} == set(w) - {"segs"}
    # ... and the comparison of the GPU test accepts it, on the twin as well
    virt = F.Virtual(lb, F.placed_of(w["segs"]))
    assert F.compare(w, {k: v for k, v in w.items() if k != "segs"}, virt.seg_same) is None


def test_the_compressed_twin_answers_as_the_document_does():
    """scan, rows, hit spans, the map and the word filter through the compressed twin against the same references over the whole
    scaled-down batch"""
    import lowermap_cases as LM
    import spans as S
    import word_cases as W
    from long_terms import brute_force
    from oracle.pyoracle import POS_END, POS_START, Oracle, pack_strings
    lb = F.long_batch(TWIN)
    docs = lb.bodies()
    cut, maps = F.compressed(TWIN)
    assert sum(map(len, cut)) < sum(map(len, docs)) and all((m is None) == (lb.docs[d].body is not None) for d, m in enumerate(maps))
    for pos_end in (False, True):
        for fold in (False, True):
            mo, ti, po = brute_force(F.TERMS, docs, POS_END if pos_end else POS_START, fold)
            assert (mo.tolist(), ti.tolist(), po.tolist()) == F.sparse_scan(pos_end, fold, TWIN)
    raw = F.sparse_scan(False, False, TWIN)
    folded = F.sparse_scan(False, True, TWIN)
    assert len(raw[1]) < len(folded[1]) and set(raw[1]) == set(range(len(F.TERMS)))        # HIT only under the fold; every keyword raw
    o = Oracle(F.TERMS)
    o.set_expressions(list(F.EXPRS), True)
    for fold in (False, True):
        blob, off = pack_strings(F.lowered_docs(docs) if fold else docs)
        rows = o.process(blob, off, fold=False)
        assert np.array_equal(rows, F.sparse_rows(fold, TWIN))
        long_rows = {int(rows[d, 0]) & 0xFF for d in lb.long_at}
        # a long document: kq; gofindthemfar and wxyz; zxq is there; wxyz in front of zxq; K33 behind K26; K300; K26 with K300; and
        # gofindthemfar behind K33 only when HIT's mixed case is lowered
        assert long_rows == {sum(int(v) << i for i, v in enumerate((1, 1, 0, 1, 0, 1, 0, fold)))}, (fold, long_rows)
    for lowered in (False, True):
        c = S.case("dense", F.EXPRS, F.lowered_docs(docs) if lowered else docs)
        total, so, st, ln, tm = S.reference(c)
        w = F.sparse_hit_spans(lowered, TWIN)
        assert (so, st, ln, tm) == (w["span_off"], w["start"], w["len"], w["term"]) and np.array_equal(c.rows, w["rows"]) and total > 20
    per = [(np.asarray(st[so[d]:so[d + 1]], np.int64), np.asarray(ln[so[d]:so[d + 1]], np.int64)) for d in range(len(docs))]
    m = LM.expected(docs, per)
    w = F.sparse_mapped(TWIN)
    assert m[1].tolist() == w["start"] and m[2].tolist() == w["len"] and (m[1].tolist() != st or m[2].tolist() != ln)
    words = F.sparse_words(TWIN)
    dense = [(d, W.kept(docs[d], a, a + n)) for d, doc in enumerate(lb.docs) for a, n, _ in doc.spans]
    assert dense == words["kept"]


def test_the_word_filter_keeps_and_drops_in_the_far_documents():
    lb = F.long_batch()
    kept = F.sparse_words()["kept"]
    for docs, what in (([lb.long_at[4]], "long_4"), (list(lb.island_docs(5)), "island 5")):
        got = {k for d, k in kept if d in docs}
        assert got == {True, False}, (what, got)


def test_every_mutant_is_noticed():
    told = F.assert_not_vacuous()
    print(told)
    assert set(told) == set(F.SPARSE)


def test_the_dictionaries_of_layer_a_have_every_length_class():
    c = pl.length_classes(pl.TERMS_ASCII)
    assert all(c[k] for k in ("1-3", "4", "5-24", "25-28", "29-40", "long"))
