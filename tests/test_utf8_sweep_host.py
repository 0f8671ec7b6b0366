"""The sweep of tests/utf8_sweep.py without a device: its numbers, that it is not vacuous, the host twins of the four UTF-8 kernels
against its plain references on its own layouts -- so that what tests/test_gpu_utf8_sweep.py holds the kernels to is known to be
right here --, and the mutants: outputs of references altered in one place, which the GPU module's comparisons must notice."""
import ctypes as C

import numpy as np
import pytest

import lowermap_cases as M
import utf8_sweep as S
import word_cases as WC
from gofindthem_amd import _lib, finder, group
from gofindthem_amd.engine import filter_word_matches_host, map_spans_to_source_host


@pytest.fixture(scope="module")
def tables():
    return S.tables()


# ---- the numbers -----------------------------------------------------------------------------------------------------------------
def test_utf8_of_is_the_interpreters_encoder():
    cp = np.concatenate([np.arange(0xD800), np.arange(0xE000, S.N_CP)]).astype(np.uint32)
    data, lens = S.utf8_of(cp)
    assert data.tobytes() == cp.astype("<u4").tobytes().decode("utf-32-le").encode("utf-8")
    assert int(lens.sum()) == data.size and S.scalars().size == 1111936


def test_tables(tables):
    lower, word = tables
    assert lower.size == word.size == S.N_CP
    assert int((lower != np.arange(S.N_CP)).sum()) == S.N_CASED
    assert lower[0x10400] == 0x10428 and lower[0x1E921] == 0x1E943 and lower[0x130] == ord("i") and word[0x1D49C] and not word[0x1F600]
    planes = np.flatnonzero(lower != np.arange(S.N_CP)) >> 16
    assert int((planes >= 1).sum()) == 225


def test_sequence_counts():
    sq, hs = S.seqs(), S.high_seqs()
    assert len(sq) == S.N_SEQS and len(set(sq.list)) == S.N_SEQS
    assert len(hs) == S.N_HIGH_SEQS and int(hs.valid.sum()) == S.N_HIGH_VALID
    assert set(hs.list) == {s for s in sq.list if min(s) >= 0x80}
    # the interpreter's strict decoder agrees on which sequences are valid
    for s, v in list(zip(hs.list, hs.valid))[::37]:
        try:
            s.decode("utf-8")
            ok = True
        except UnicodeDecodeError:
            ok = False
        assert ok == bool(v), S.hexs(s)


def test_l3_sizes():
    b = S.l3(False)
    assert b.blob.tobytes() == b"Z".join(S.seqs().list) + b"Z"
    assert b.blob.size == S.L3_BYTES and b.want.size == S.L3_LOWERED
    d = S.l3(True)
    assert d.n_docs == 2 * S.N_SEQS and d.want.size == S.L3_LOWERED - S.N_SEQS + 9 * S.N_SEQS
    docs = S.as_list((d.blob, np.diff(d.doc_off.astype(np.int64))))
    assert docs[0::2] == S.seqs().list and set(docs[1::2]) == {S.TAIL}


def test_word_cell_counts():
    w = S.words(False)
    ab = w.keep.reshape(-1, 3)[:, :2]
    assert ab.size == S.W_AB_CELLS and int(ab.sum()) == S.W_AB_KEPT
    assert np.array_equal(w.keep, S.words(True).keep)


def test_not_vacuous():
    S.assert_not_vacuous()


def test_finder_case(tables):
    lower, word = tables
    f = S.FinderCase()
    assert f.n_cased == S.N_CASED and len(f.keywords) == 1384 + 1 and f.keywords[-1] == "x" and f.keywords.count("x") == 2
    assert np.array_equal(lower[f.runes], f.runes), "a lower form that is not its own lower form"
    assert np.array_equal(word[f.low], word[f.cp]), "lowering moved a code point over the word border"
    plain, whole = f.hits(False), f.hits(True)
    docs = S.as_list((f.blob, np.diff(f.doc_off.astype(np.int64))))
    for d in list(range(0, len(docs), 211)) + [int(np.flatnonzero(f.cp == 0x10400)[0])]:
        text = docs[d].decode("utf-8")
        low = "x" + chr(int(lower[ord(text[1])])) + "y"
        assert [k in low for k in f.keywords] == plain[d].tolist(), text
    assert plain[:, -1].all() and int(plain[:f.n_cased, :-1].sum()) == 3 * f.n_cased - 2
    # with whole words `x` hits exactly the documents whose code point is no word rune, and some of those are cased
    assert np.array_equal(whole[:, -1], ~word[f.cp]) and 0 < int(whole[:f.n_cased, -1].sum()) < 100 < int(whole[:, -1].sum())


# ---- strings.ToLower ---------------------------------------------------------------------------------------------------------------
def emulate(batch):
    """gft_debug_emulate_to_lower over a batch -> (out, out_off, total)"""
    L = _lib.load()
    out_off = np.full(batch.n_docs + 1, 0xDEAD, np.uint64)
    total = C.c_uint64(0)
    blob = np.ascontiguousarray(batch.blob)
    assert L.gft_debug_emulate_to_lower(blob.ctypes.data, batch.doc_off.ctypes.data, batch.n_docs, None, 0, out_off.ctypes.data, C.byref(total)) == 0
    out = np.full(total.value + 1, 0xA5, np.uint8)
    assert L.gft_debug_emulate_to_lower(blob.ctypes.data, batch.doc_off.ctypes.data, batch.n_docs, out.ctypes.data, total.value, out_off.ctypes.data,
                                        C.byref(total)) == 0
    assert out[total.value] == 0xA5
    return out[:total.value], out_off, total.value


@pytest.mark.parametrize("name", ["L3 in one document", "L3 per document", "L1 at three shifts"])
def test_to_lower_twins(name):
    b = {"L3 in one document": lambda: S.l3(False), "L3 per document": lambda: S.l3(True), "L1 at three shifts": lambda: S.l1([0, 5, 15])}[name]()
    S.check_lower(b, *emulate(b))
    if b.n_docs <= 3:                                                # gft_to_lower, document by document
        off = b.doc_off.astype(np.int64)
        low = [S.host_lower(b.blob[off[d]:off[d + 1]]) for d in range(b.n_docs)]
        S.check_lower(b, np.concatenate(low), np.concatenate([[0], np.cumsum([x.size for x in low])]), sum(x.size for x in low))


def test_to_lower_of_every_sequence_alone():
    """gft_to_lower sees each sequence of SEQS with nothing behind it: every 5th, and every one that ends in a cut lead"""
    sq = S.seqs()
    low = S.as_list(sq.lowered(S.tables()[0])[0])
    for i in sorted(set(range(0, len(sq), 5)) | set(np.flatnonzero(sq.last < 0)[::3].tolist())):
        assert S.host_lower(np.frombuffer(sq.list[i], np.uint8)).tobytes() == low[i], sq.label(i)


# ---- spans mapped back -------------------------------------------------------------------------------------------------------------
def host_map(b, so, st, ln):
    st, ln = st.astype(np.uint32), ln.astype(np.uint32)
    map_spans_to_source_host(b.blob, b.doc_off, so, st, ln)
    return st, ln


@pytest.mark.parametrize("per_document", [False, True], ids=["one document", "per document"])
def test_map_spans_twin_on_l3(per_document):
    b = S.l3(per_document)
    so, st, ln, w_st, w_ln = b.spans()
    assert st.size == int(S.seqs().n_runes.sum()) > 800000
    S.check_spans(b, *host_map(b, so, st, ln), w_st, w_ln)


def test_map_spans_twin_against_the_sequential_reference():
    """every 7th sequence, in both forms, through lowermap_cases.expected"""
    for per_document in (False, True):
        b = S.l3(per_document, every=7)
        so, st, ln, w_st, w_ln = b.spans()
        off = b.doc_off.astype(np.int64)
        raw = b.blob.tobytes()
        docs = [raw[off[d]:off[d + 1]] for d in range(b.n_docs)]
        s = so.astype(np.int64)
        ref = M.expected(docs, [(st[s[d]:s[d + 1]], ln[s[d]:s[d + 1]]) for d in range(b.n_docs)])
        S.check_spans(b, ref[1], ref[2], w_st, w_ln)
        S.check_spans(b, *host_map(b, so, st, ln), ref[1], ref[2])


def test_map_spans_twin_on_l1_and_l2():
    for b in (S.l1([5]), S.l2()):
        so, st, ln, w_st, w_ln = b.spans()
        S.check_spans(b, *host_map(b, so, st, ln), w_st, w_ln)


# ---- the word filter -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[False, True], ids=["large documents", "per document"])
def words(request):
    return S.words(request.param)


def test_word_cells_obey_the_rule_of_word_cases(words, tables, monkeypatch):
    """word_cases.kept itself, with WORD in place of CLASS, on every 29th entry of the layout as it lies in its document"""
    monkeypatch.setattr(WC, "CLASS", tables[1])
    w = words
    raw, off = w.blob.tobytes(), w.doc_off.astype(np.int64)
    for e in list(range(0, w.n, 29)) + list(range(w.n - 3 * S.N_SEQS, w.n, 3 * 997)):
        d = int(w.entry_doc[e])
        s = int(off[d]) + int(w.pos[e])
        lo, hi = max(int(off[d]), s - 8), min(int(off[d + 1]), s + int(w.length[e]) + 8)
        assert WC.kept(raw[lo:hi], s - lo, s - lo + int(w.length[e])) == bool(w.keep[e]), w.label(e)


@pytest.mark.parametrize("from_terms,pos_end", [(True, False), (False, True)], ids=["term_len", "lengths, last bytes"])
def test_word_filter_twin(words, from_terms, pos_end):
    w = words
    got = filter_word_matches_host(w.blob, w.doc_off, w.off, w.pos_for(pos_end), None if from_terms else w.length, w.term,
                                   w.term_len if from_terms else None, pos_end)
    S.check_words(w, *got, pos_end=pos_end)


# ---- JSON ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grp():
    f = finder.Finder(None, None, False, allow_no_device=True)
    g = group.NewFinderWithRules(f, {})
    g.SetSchema(["a"])
    g._keep = f
    return g


J_CASES = [("escapes", p) for p in S.J_ESCAPE_PADS] + [("high", p) for p in S.J_HIGH_PADS] + [("raw", 0)]


def make_json(kind, pad):
    return S.json_escapes(pad) if kind == "escapes" else S.json_high(pad) if kind == "high" else S.json_raw()


@pytest.mark.parametrize("kind,pad", J_CASES, ids=["%s-%d" % c for c in J_CASES])
def test_json_twins(grp, kind, pad):
    j = make_json(kind, pad)
    docs = j.docs()
    ref = grp.debug_json_leaves_ref(docs)
    emu = grp.debug_emulate_json_leaves(docs)
    for x, y, what in zip(ref[:5], emu[:5], ("status", "rec_off", "leaf_field", "leaf_off", "text")):
        assert np.array_equal(x, y), (j.name, what)
    assert ref[5] == emu[5]
    S.check_json(j, *emu)
    if kind == "escapes":                                            # the OK texts against chr(v)
        text, off = emu[4].tobytes(), emu[3].astype(np.int64)
        ok = np.flatnonzero(emu[0] == S.J_OK)
        for k in range(0, ok.size, 61):
            assert text[off[k]:off[k + 1]] == b"p" * pad + chr(int(ok[k]) // 2).encode("utf-8"), j.label(int(ok[k]))
        assert docs[2 * 0xABCD] == S.J_HEAD + b"p" * pad + b"\\uabcd" + S.J_TAIL and docs[2 * 0xABCD + 1].endswith(b"\\uABCD" + S.J_TAIL)
        assert len(S.J_HEAD) + pad in (6, 58, 59, 60, 61, 62, 63)


# ---- the mutants -----------------------------------------------------------------------------------------------------------------
def decode_rune_with_surrogates(p):
    """word_cases.decode_rune, but ED A0..BF 80..BF is taken as valid"""
    if len(p) >= 3 and p[0] == 0xED and 0xA0 <= p[1] <= 0xBF and 0x80 <= p[2] <= 0xBF:
        return (0xD000 | (p[1] & 0x3F) << 6 | (p[2] & 0x3F)), 3
    return WC.decode_rune(p)


def json_outputs(j):
    """what a walker that followed the reference j would return"""
    n = int(j.rec_off[-1])
    return j.status, j.rec_off, np.zeros(n, np.uint32), j.text_off, j.text, (n, int(j.text_off[-1]))


def test_mutant_lower_entry_in_plane_1(tables):
    lower = tables[0].copy()
    lower[0x1E921] = 0x1E921
    for good, bad in ((S.l1([0, 5]), S.l1([0, 5], lower)), (S.l2(), S.l2(lower))):
        S.check_lower(good, good.want, good.want_off, good.want.size)
        with pytest.raises(AssertionError, match="U\\+1E921"):
            S.check_lower(good, bad.want, bad.want_off, bad.want.size)
    # a changed length moves the offsets; a span of one byte too few comes back one rune short
    lower[0x10400] = 0x2C65
    good, bad = S.l2(), S.l2(lower)
    with pytest.raises(AssertionError, match="U\\+10400"):
        S.check_lower(good, bad.want, bad.want_off, bad.want.size)
    g = good.spans()
    S.check_spans(good, g[3], g[4], g[3], g[4])
    k = 2 * int(np.flatnonzero(good.cp == 0x10400)[0])
    short = g[4].copy()
    short[k] -= 1
    with pytest.raises(AssertionError, match="U\\+10400"):
        S.check_spans(good, g[3], short, g[3], g[4])
    # the finder: U+10400 lowered to its neighbour's lower form
    f, f2 = S.FinderCase(), S.FinderCase()
    S.check_hits(f, f.hits())
    f2.low = f2.low.copy()
    f2.low[f2.cp == 0x10400] = 0x10429
    with pytest.raises(AssertionError, match="U\\+10400"):
        S.check_hits(f, f2.hits())


def test_mutant_word_bit_in_plane_1(tables):
    word = tables[1].copy()
    word[0x1D49C] = False
    for per_document in (False, True):
        good, bad = S.words(per_document), S.Words(per_document, word=word)
        S.check_words(good, good.reference()[1].size, *good.reference())
        with pytest.raises(AssertionError, match="U\\+1D49C"):
            S.check_words(good, bad.reference()[1].size, *bad.reference())
    f = S.FinderCase()
    cp = int(f.cp[(f.cp >= 0x10000) & ~word[f.cp]][0])
    word[cp] = True
    S.check_hits(f, f.hits(True), True)
    with pytest.raises(AssertionError, match="whole words True: document U\\+%04X and keyword 'x'" % cp):
        S.check_hits(f, S.FinderCase(word=word).hits(True), True)


def test_mutant_surrogate_taken_as_valid():
    bad_sq = S.Seqs(S.make_seqs(False), decode=decode_rune_with_surrogates)
    for per_document in (False, True):
        good, bad = S.l3(per_document), S.l3(per_document, bad_sq)
        with pytest.raises(AssertionError, match="sequence ed a0 80"):
            S.check_lower(good, bad.want, bad.want_off, bad.want.size)
        g, b = good.spans(), bad.spans()
        S.check_spans(good, g[3], g[4], g[3], g[4])
        with pytest.raises(AssertionError, match="sequence ed a0"):
            S.check_spans(good, b[3][:g[3].size], b[4][:g[4].size], g[3], g[4])
    bad_hs = S.Seqs(S.make_seqs(True), decode=decode_rune_with_surrogates)
    good = S.json_high(56)
    S.check_json(good, *json_outputs(good))
    with pytest.raises(AssertionError, match="sequence ed a0 80"):
        S.check_json(good, *json_outputs(S.json_high(56, valid=bad_hs.valid)))


def test_mutant_decode_last_rune_accepts_a_cut_sequence(tables):
    """E2 82 in front of `ab` taken for U+2080, a digit: DecodeLastRune went on where the sequence was cut"""
    sq = S.seqs()
    last = sq.last.copy()
    i = sq.list.index(b"\xe2\x82")
    assert last[i] == -1 and tables[1][0x2080]
    last[i] = 0x2080
    for per_document in (False, True):
        good, bad = S.words(per_document), S.Words(per_document, last=last)
        with pytest.raises(AssertionError, match="cell A of sequence e2 82 "):
            S.check_words(good, bad.reference()[1].size, *bad.reference())


def test_mutant_escape_loses_its_last_digit():
    good, bad = S.json_escapes(55), S.json_escapes(55, value_of=lambda v: v >> 4)
    S.check_json(good, *json_outputs(good))
    with pytest.raises(AssertionError, match="escapes at pad 55: .*: .ud800$"):
        S.check_json(good, *json_outputs(bad))
