"""The four device kernels that decode UTF-8 or read a Unicode table, on every code point and every short byte sequence
(tests/utf8_sweep.py; the references and the comparisons are held to the host library by tests/test_utf8_sweep_host.py):
gft_to_lower_device and the table form of k_lower behind gft_map_spans_to_source_device, gft_filter_word_matches_device,
gft_group_json_leaves_device, and the finder's lowered route on top of the first.  All comparisons are exact; a mismatch names the
first differing code point or sequence in hex.  The largest batch, L1, is 70 MB of text."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before libgft.so is loaded: one HIP runtime)

import utf8_sweep as S
from gofindthem_amd import _lib, group
from gofindthem_amd.engine import Engine, map_spans_to_source_host
from gofindthem_amd.finder import EmptyRgxEngine, Finder, GpuEngine
from json_docs import check_leaves, to_device

pytestmark = pytest.mark.gpu

GUARD = 256
G32, G64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def eng():
    e = Engine()
    yield e
    e.close()


@pytest.fixture(scope="module", autouse=True)
def device_memory():
    """prints what the module held at most in torch's allocator, and what the device had in use at its end"""
    torch.cuda.reset_peak_memory_stats()
    yield
    free, total = torch.cuda.mem_get_info()
    print("\nutf8 sweep: peak of torch's allocator %.0f MB, device memory in use at the end %.0f MB" % (
        torch.cuda.max_memory_allocated() / 2**20, (total - free) / 2**20))


def dev(a):
    """a numpy array on the device, unsigned integers as the signed type of their size (an empty one gets a word: an address)"""
    a = np.ascontiguousarray(a)
    signed = a.view({1: np.uint8, 4: np.int32, 8: np.int64}[a.dtype.itemsize])
    return torch.from_numpy(np.concatenate([signed.ravel(), np.zeros(1, signed.dtype)])).cuda()[:a.size]


def place(blob, lead=0, at=0, fill=(0xC3, 0x89)):
    """the text on the device: `lead` bytes that would lead its first rune in front, 64 that would continue its last one behind,
    the whole `at` bytes into its allocation"""
    buf = np.concatenate([np.full(at + lead, fill[0], np.uint8), blob, np.full(64, fill[1], np.uint8)])
    return torch.from_numpy(buf).cuda()[at:]


BATCHES = {"L1": lambda: S.l1(), "L2": lambda: S.l2(), "L3 in one document": lambda: S.l3(False), "L3 per document": lambda: S.l3(True),
           "L1 at shifts 0, 5 and 15": lambda: S.l1([0, 5, 15])}


# ---- gft_to_lower_device -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,lead", [("L1", 0), ("L2", 0), ("L2", 5), ("L3 in one document", 0), ("L3 in one document", 5),
                                       ("L3 per document", 0), ("L3 per document", 5)])
def test_to_lower(eng, name, lead):
    """the count-only call, then the writing call into a guarded buffer: bytes, out_off and total against the reference"""
    b = BATCHES[name]()
    text, off = place(b.blob, lead), dev(b.doc_off + np.uint64(lead))
    out_off = torch.full((b.n_docs + 1,), 0x5A5A, dtype=torch.int64, device="cuda")
    total = eng.to_lower_device(text.data_ptr(), off.data_ptr(), b.n_docs, None, 0, out_off.data_ptr())
    S.check_lower(b, None, out_off.cpu().numpy().view(np.uint64), total)
    out = torch.full((total + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    out_off.fill_(0x5A5A)
    assert eng.to_lower_device(text.data_ptr(), off.data_ptr(), b.n_docs, out.data_ptr(), total, out_off.data_ptr()) == total
    got = out.cpu().numpy()
    S.check_lower(b, got[:total], out_off.cpu().numpy().view(np.uint64), total)
    assert (got[total:] == 0xA5).all(), "bytes stored past the cap"


# ---- gft_map_spans_to_source_device ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["L1 at shifts 0, 5 and 15", "L2", "L3 in one document", "L3 per document"])
def test_map_spans_to_source(eng, name):
    """L1 and L2: a span over each lowered rune and one on its last lowered byte alone come back as the source rune; L3: a span over
    each lowered rune against the host walk, which is the reference's"""
    b = BATCHES[name]()
    so, st, ln, w_st, w_ln = b.spans()
    st, ln = st.astype(np.uint32), ln.astype(np.uint32)
    if name.startswith("L3"):
        h_st, h_ln = st.copy(), ln.copy()
        map_spans_to_source_host(b.blob, b.doc_off, so, h_st, h_ln)
        S.check_spans(b, h_st, h_ln, w_st, w_ln)
    text, d_off, d_so, d_st, d_ln = place(b.blob), dev(b.doc_off), dev(so), dev(st), dev(ln)
    eng.map_spans_to_source_device(text, d_off, d_so, d_st, d_ln)
    S.check_spans(b, d_st.cpu().numpy(), d_ln.cpu().numpy(), w_st, w_ln)


# ---- gft_filter_word_matches_device ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[False, True], ids=["large documents", "per document"])
def words(request):
    w = S.words(request.param)
    return w, {k: dev(getattr(w, k)) for k in ("doc_off", "off", "length", "term", "term_len")}


@pytest.mark.parametrize("pos_end", [False, True], ids=["first bytes", "last bytes"])
def test_filter_word_matches(eng, words, pos_end):
    """both length sources, the text 0 and 3 bytes into its allocation: out_off, pos, len and term against the rule"""
    w, d = words
    L = _lib.load()
    d_pos = dev(w.pos_for(pos_end))
    want_total = int(w.keep.sum())
    for at in (0, 3):
        text = place(w.blob[:-64], at=at, fill=(ord("a"), ord("a")))
        for from_terms in (True, False):
            args = (eng._h, text.data_ptr(), d["doc_off"].data_ptr(), w.n_docs, d["off"].data_ptr(), d_pos.data_ptr(),
                    None if from_terms else d["length"].data_ptr(), d["term"].data_ptr(), d["term_len"].data_ptr() if from_terms else None,
                    w.term_len.size if from_terms else 0, 1 if pos_end else 0)
            total = C.c_uint64(0)
            torch.cuda.synchronize()
            assert L.gft_filter_word_matches_device(*args, None, None, None, None, 0, C.byref(total)) == 0, eng._L.gft_last_error(eng._h)
            assert int(total.value) == want_total, "%s: the count-only call kept %d, not %d" % (w.name, int(total.value), want_total)
            cap = int(total.value)
            out_off = dev(np.full(w.n_docs + 1 + 2, G64, np.uint64))
            outs = [dev(np.full(cap + 2, G32, np.uint32)) for _ in range(3)]
            assert L.gft_filter_word_matches_device(*args, out_off.data_ptr(), *(o.data_ptr() for o in outs), cap, C.byref(total)) == 0
            torch.cuda.synchronize()
            oo = out_off.cpu().numpy().view(np.uint64)
            back = [o.cpu().numpy().view(np.uint32) for o in outs]
            S.check_words(w, int(total.value), oo, *back, pos_end=pos_end)
            assert (oo[w.n_docs + 1:] == G64).all() and all((x[cap:] == G32).all() for x in back), "stored behind the caps"


# ---- gft_group_json_leaves_device --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grp():
    f = Finder(GpuEngine(), EmptyRgxEngine(), False)
    f.AddExpressionWithTag('"x"', "t")
    g = group.NewFinderWithRules(f, {})
    g.SetSchema(["a"])
    return g


RAW_PARTS = 4
J_CASES = [("escapes", p, 0) for p in S.J_ESCAPE_PADS] + [("high", p, 0) for p in S.J_HIGH_PADS] + [("raw", 0, k) for k in range(RAW_PARTS)]


@pytest.mark.parametrize("kind,pad,part", J_CASES, ids=["%s-%d-%d" % c for c in J_CASES])
def test_json_leaves(grp, kind, pad, part):
    """status and text against the expected values themselves, then every array against the host reader"""
    j = S.json_escapes(pad) if kind == "escapes" else S.json_high(pad) if kind == "high" else S.json_raw(part, RAW_PARTS)
    docs = j.docs()
    status, rec_off, leaf_field, leaf_off, text, totals = grp.JsonLeavesDevice(*to_device(docs))
    S.check_json(j, *(t.cpu().numpy() for t in (status, rec_off, leaf_field, leaf_off, text)), totals)
    check_leaves(grp, docs)


# ---- the finder's lowered route ----------------------------------------------------------------------------------------------------
def test_finder_lowered_route():
    """one expression per keyword, case-insensitive, over the documents x<cp>y: the hit matrix; then with whole words"""
    case = S.FinderCase()
    f = Finder(GpuEngine.__new__(GpuEngine), EmptyRgxEngine(), False)
    try:
        f.AddExpressions(['"%s"' % k for k in case.keywords])
        n, n_exprs = case.cp.size, len(case.keywords)
        text, off = place(case.blob), dev(case.doc_off)
        for whole in (False, True):
            f.whole_words = whole
            before = f.lowered_batches()
            bm = torch.zeros((n, (n_exprs + 31) // 32), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            f.ProcessDevice(text.data_ptr(), off.data_ptr(), n, bm.data_ptr())
            after = f.lowered_batches()
            assert (after[0] - before[0], after[1] - before[1]) == (1, 0), "the batch was not lowered on the device"
            S.check_hits(case, S.unpack_rows(bm.cpu().numpy().view(np.uint32), n_exprs), whole)
    finally:
        f.close()
