"""Spans of a lowered batch mapped back to the source text, on the host: gft_debug_map_spans_to_source -- the kernels' table build
and span map walked unit by unit, piece by piece and span by span through the headers they compile -- against the sequential
reference of lowermap_cases.py.  Every lowered byte of every document of the ToLower batches, the piece, trip and unit borders,
placement, the degenerate shapes, identity on fold-safe text and the refusals.  All comparisons are exact; no device needed."""
import numpy as np
import pytest

import lowermap_cases as M
import tolower_cases as TC
from gofindthem_amd import _lib
from gofindthem_amd.engine import GftError, lowermap_shape, map_spans_to_source_host


def host_map(docs, spans, lead=0):
    blob, off = TC.pack(list(docs), lead)
    so, st, ln = M.flat(spans)
    map_spans_to_source_host(blob, off, so, st, ln)
    return so, st, ln


def assert_maps(docs, spans, lead=0, what=""):
    want = M.expected(docs, spans)
    assert want is not None
    got = host_map(docs, spans, lead)
    for g, w, name in zip(got, want, ("span_off", "start", "len")):
        if not np.array_equal(g, w):
            k = int(np.nonzero(g != w)[0][0])
            raise AssertionError("%s: %s differs first at %d: got %d, want %d" % (what, name, k, g[k], w[k]))


def refused(blob, off, so, st, ln):
    """the call is refused with GFT_E_INVALID and both arrays keep every byte"""
    a, b = st.copy(), ln.copy()
    with pytest.raises(GftError) as ei:
        map_spans_to_source_host(blob, off, so, st, ln)
    assert ei.value.code == _lib.GFT_E_INVALID
    assert st.tobytes() == a.tobytes() and ln.tobytes() == b.tobytes()


def test_symbols_present():
    L = _lib.load()
    for name in ("gft_map_spans_to_source_device", "gft_debug_map_spans_to_source", "gft_debug_lowermap_shape",
                 "gft_finder_hit_spans_source_device"):
        assert hasattr(L, name) and name in _lib.SYMBOLS
    assert lowermap_shape() == (TC.PIECE, TC.CHUNK, TC.UNIT_MAX, 64)


def test_the_reference_is_pinned_to_to_lower():
    """the concatenated lowered runes are gft_to_lower of the document, for every document any test here uses"""
    docs = [d for b in TC.edge_batches().values() for d in b] + TC.random_docs() + [d for d, _ in M.border_docs()] + M.fold_safe_docs()
    for d in docs:
        r = M.runes(d)
        assert r.lowered == TC.ref_lower(d), d[:40]
        assert int(r.sl.sum()) == len(d) and int(r.ll.sum()) == len(r.lowered) and (r.ll >= 1).all()


@pytest.mark.parametrize("name", sorted(TC.edge_batches()))
def test_every_lowered_byte_of_the_edge_batches(name):
    docs = TC.edge_batches()[name]
    assert_maps(docs, [M.every_byte(d, seed=i) for i, d in enumerate(docs)], what=name)


def test_every_lowered_byte_of_random_documents():
    docs = TC.random_docs()
    spans = [M.every_byte(d, seed=i) for i, d in enumerate(docs)]
    assert_maps(docs, spans, what="random")
    # the batch is not vacuous: some span moves, some grows to cover a cut rune
    so, st, ln = M.flat(spans)
    w = M.expected(docs, spans)
    assert (w[1] != st).any() and (w[2] > ln).any() and (w[2] < ln).any()


@pytest.mark.parametrize("border", sorted(M.borders()))
def test_runes_at_the_borders(border):
    placed = M.border_docs([border])
    assert len(placed) >= 50
    docs = [d for d, _ in placed]
    assert_maps(docs, [M.around(d, at) for d, at in placed], what=border)
    if border == "unit cut":                                        # (the cut the kernels make is where this file says it is)
        k, n = M.borders()[border]
        assert n > TC.UNIT_MAX and k == (n + 1) // 2 and all(len(d) == n for d in docs)


def test_placement_lead_bytes_and_slack_do_not_matter():
    """doc_off[0] != 0; the lead bytes (0xC3) and the slack (0x89) would complete the runes the batch's ends cut"""
    docs = [b"\xa9 starts with a continuation byte", "CAFÉ İK".encode(), b"", "Ⱥ".encode() * 40, b"ends with a lead byte \xc3"]
    spans = [M.every_byte(d, seed=i) for i, d in enumerate(docs)]
    for lead in (0, 1, 3, 16, 29):
        assert_maps(docs, spans, lead, what="lead %d" % lead)
    # ... and neighbours inside the batch do not complete each other either
    docs = [b"ab\xc3", b"\x89cd\xe2\x82", b"\xac!", b"\xf0\x9f", b"\x98\x80"]
    assert_maps(docs, [M.every_byte(d) for d in docs], 5, what="cut neighbours")


def test_degenerate_shapes():
    one = np.zeros(1, np.int64)
    # the empty document and a document of one byte, zero-length spans, at the lowered end too
    docs = [b"", b"K", b"\xff", "İ".encode()]
    spans = [(one, one), (np.array([0, 0, 1]), np.array([1, 0, 0])), (np.array([0, 1, 2, 3, 0]), np.array([0, 0, 0, 0, 3])),
             (np.array([0, 1, 0]), np.array([0, 0, 1]))]
    assert_maps(docs, spans, what="tiny")
    so, st, ln = host_map(docs, spans)
    assert st.tolist() == [0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 2, 0] and ln.tolist() == [0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 2]
    # no spans at all; no documents
    none = (np.zeros(0, np.int64), np.zeros(0, np.int64))
    assert_maps(docs, [none] * 4, what="no spans")
    assert_maps([], [], what="no documents")
    # 130 spans in one document: more than two wave tiles; 130 documents with a span each
    d = ("İstanbul Ⱥ KELVIN K ".encode() + b"\xff ") * 12 + "İK".encode() * 30
    s = np.arange(130) % M.lowered_len(d)
    assert_maps([b"x", d, b""], [none, (s, np.ones(130, np.int64)), none], what="130 spans")
    docs = [("É%d İ" % i).encode() for i in range(130)]
    assert_maps(docs, [(np.array([i % 3]), np.array([2])) for i in range(130)], what="130 documents")


def test_identity_on_fold_safe_documents():
    docs = M.fold_safe_docs()
    spans = []
    for i, d in enumerate(docs):
        cuts = np.concatenate([M.runes(d).a, [len(d)]])            # spans from rune cut to rune cut
        rng = np.random.default_rng(i)
        x = np.sort(rng.integers(0, cuts.size, size=(60, 2)), axis=1)
        spans.append((cuts[x[:, 0]], cuts[x[:, 1]] - cuts[x[:, 0]]))
    so, st, ln = M.flat(spans)
    got = host_map(docs, spans)
    assert np.array_equal(got[1], st) and np.array_equal(got[2], ln) and st.size == 360
    assert_maps(docs, spans, what="identity")
    # in ASCII every span is its own image, inside "runes" or not
    d = TC._ascii(5000, 9)
    s, n = M.every_byte(d)
    got = host_map([d], [(s, n)])
    assert np.array_equal(got[1], s.astype(np.uint32)) and np.array_equal(got[2], n.astype(np.uint32))


def test_refusals_write_nothing():
    docs = ["CAFÉ İ one".encode(), "İİ two Ⱥ".encode(), b"three \xff"]
    Bs = [M.lowered_len(d) for d in docs]
    good = [(np.array([0, 2]), np.array([3, 1]))] * 3
    for bad_doc in (2, 1):                                          # the last document, a middle one
        spans = list(good)
        spans[bad_doc] = (np.array([0, Bs[bad_doc] - 1, 1]), np.array([1, 2, 1]))      # start + len == B + 1
        assert M.expected(docs, spans) is None
        blob, off = TC.pack(docs)
        refused(blob, off, *M.flat(spans))
        spans[bad_doc] = (np.array([0, Bs[bad_doc] + 1, 1]), np.array([1, 0, 1]))      # an empty span behind the end
        refused(blob, off, *M.flat(spans))
    blob, off = TC.pack(docs)
    so, st, ln = M.flat(good)
    # overlapping arrays: the two span arrays; a span array and the offsets
    both = np.concatenate([st, ln[1:]])
    refused(blob, off, so, both[:st.size], both[st.size - 1:])
    refused(blob, off, so, off.view(np.uint32)[:st.size], ln)
    assert np.array_equal(off, TC.pack(docs)[1])
    # descending offsets: of the documents, of the spans
    down = off.copy()
    down[1], down[2] = off[2], off[1]
    refused(blob, down, so, st, ln)
    sdown = so.copy()
    sdown[1], sdown[2] = so[2], so[1]
    refused(blob, off, sdown, st, ln)
    # and the same arrays map when nothing is wrong with them
    map_spans_to_source_host(blob, off, so, st, ln)
    w = M.expected(docs, good)
    assert np.array_equal(st, w[1]) and np.array_equal(ln, w[2])
