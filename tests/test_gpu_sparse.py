"""Sparse batch results on the GPU: the device compaction (gft_compact.hip behind gft_compact_device) against numpy and
against its host restatement, and the finder's sparse batch entry points against the reference's fixtures and the oracle's
per-document solve -- device route and host route (regex terms, host-solved expressions, text that leaves ASCII), two
batches in flight, a handle over several devices."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before libgft.so is loaded: both must share ONE HIP runtime, the one torch brings along)

from conftest import load_golden
from gofindthem_amd import _lib
from gofindthem_amd.engine import Engine, GftError, compact_host
from gofindthem_amd.finder import EmptyRgxEngine, Finder, FinderError, GpuEngine, PyRegexpEngine
from gofindthem_amd.workload import Workload, make_expressions
from oracle.pyoracle import Oracle, pack_strings
from test_host_logic import make_mocked_finder
from test_sparse_host import DENSITY, N_DOCS, N_EXPRS, make_labels, numpy_csr

pytestmark = pytest.mark.gpu

CANARY = 0x5EEDCAFE


def device_bitmap(n_docs, n_exprs, density, seed):
    """a bitmap made with torch on the device (junk in the padding bits of every row's last word), as uint32 numpy rows"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    words = (n_exprs + 31) // 32
    if density <= 0:
        bits = torch.zeros((n_docs, words * 32), dtype=torch.bool, device="cuda")
    elif density >= 1:
        bits = torch.ones((n_docs, words * 32), dtype=torch.bool, device="cuda")
    else:
        bits = torch.rand((n_docs, words * 32), generator=g, device="cuda") < density
    if words * 32 > n_exprs:
        bits[:, n_exprs:] = torch.rand((n_docs, words * 32 - n_exprs), generator=g, device="cuda") < 0.5
    weights = 2 ** torch.arange(32, dtype=torch.int64, device="cuda")
    bm = (bits.view(n_docs, words, 32).to(torch.int64) * weights).sum(dim=2)
    return bm.cpu().numpy().astype(np.uint32)


def engine_with(n_exprs, labels=None):
    """an engine whose programs give rows of n_exprs bits (every program: one term)"""
    e = Engine(0)
    e.build([b"aa", b"bb"])
    e.set_programs([[1 << 28 | (i & 1)] for i in range(n_exprs)])
    if labels is not None:
        e.set_expr_labels(labels)
    return e


def _canaries(n):
    return torch.from_numpy(np.full(n, CANARY, np.uint32).view(np.int32)).cuda()


def compact(e, bm_np, n_docs, cap, with_labels, want_total=True, slack=64):
    """gft_compact_device on a copy of bm_np in device memory -> (row_off, expr_idx, label, total) as numpy; the result
    buffers are `slack` entries longer than cap and filled with a canary"""
    d_bm = torch.from_numpy(bm_np.view(np.int32).reshape(-1).copy()).cuda() if bm_np.size else torch.zeros(1, dtype=torch.int32, device="cuda")
    d_ro = torch.full((n_docs + 1,), -1, dtype=torch.int64, device="cuda")
    d_ei = _canaries(cap + slack)
    d_lb = _canaries(cap + slack) if with_labels else None
    total = e.compact_device(d_bm.data_ptr(), n_docs, d_ro.data_ptr(), d_ei.data_ptr() if cap else None,
                             d_lb.data_ptr() if with_labels else None, cap, want_total=want_total)
    torch.cuda.synchronize()
    ro = d_ro.cpu().numpy().astype(np.uint64)
    ei = d_ei.cpu().numpy().view(np.uint32)
    lb = d_lb.cpu().numpy().view(np.uint32) if with_labels else None
    return ro, ei, lb, total


@pytest.mark.parametrize("n_exprs", N_EXPRS)
def test_device_compaction_equals_numpy_and_the_host_restatement(n_exprs):
    labels = make_labels(n_exprs)
    e = engine_with(n_exprs, labels)
    for n_docs in N_DOCS:
        for density in DENSITY:
            bm = device_bitmap(n_docs, n_exprs, density, seed=n_exprs * 7919 + n_docs)
            want = numpy_csr(bm, n_exprs, labels)
            total = int(want[0][-1])
            what = "n_exprs=%d n_docs=%d density=%g" % (n_exprs, n_docs, density)
            # count only
            ro, _, _, t = compact(e, bm, n_docs, 0, False)
            assert t == total and np.array_equal(ro, want[0]), what
            for with_labels in (True, False):
                ro, ei, lb, t = compact(e, bm, n_docs, total, with_labels)
                assert t == total and np.array_equal(ro, want[0]), what
                assert np.array_equal(ei[:total], want[1]), what
                assert (ei[total:] == CANARY).all(), what
                if with_labels:
                    assert np.array_equal(lb[:total], want[2]) and (lb[total:] == CANARY).all(), what
            # the host restatement gives the same arrays
            hro, hei, hlb, ht = compact_host(bm, n_exprs, labels)
            assert ht == total and np.array_equal(hro, ro) and np.array_equal(hei, ei[:total]) and np.array_equal(hlb, want[2]), what
    e.close()


def test_device_compaction_at_200k_documents_by_1000_expressions():
    n_docs, n_exprs = 200_000, 1000
    labels = make_labels(n_exprs)
    e = engine_with(n_exprs, labels)
    bm = device_bitmap(n_docs, n_exprs, 0.01, seed=3)
    want = numpy_csr(bm, n_exprs, labels)
    total = int(want[0][-1])
    assert total > n_docs
    ro, ei, lb, t = compact(e, bm, n_docs, total, True)
    assert t == total and np.array_equal(ro, want[0])
    assert np.array_equal(ei[:total], want[1]) and np.array_equal(lb[:total], want[2])
    assert (ei[total:] == CANARY).all() and (lb[total:] == CANARY).all()
    hro, hei, hlb, ht = compact_host(bm, n_exprs, labels)
    assert ht == total and np.array_equal(hro, ro) and np.array_equal(hei, ei[:total]) and np.array_equal(hlb, lb[:total])
    e.close()


@pytest.mark.parametrize("n_exprs,n_docs", [(33, 65), (1000, 1000), (2049, 64), (5000, 63)])
def test_cap_below_total(n_exprs, n_docs):
    labels = make_labels(n_exprs)
    e = engine_with(n_exprs, labels)
    bm = device_bitmap(n_docs, n_exprs, 0.5, seed=11)
    want = numpy_csr(bm, n_exprs, labels)
    total = int(want[0][-1])
    for cap in (1, total // 3, total - 1):
        # (the buffers hold the whole answer and more: a kernel that ignored cap fails the comparison, it stores nowhere else)
        ro, ei, lb, t = compact(e, bm, n_docs, cap, True, slack=total + 64)
        assert t == total and np.array_equal(ro, want[0])
        assert np.array_equal(ei[:cap], want[1][:cap]) and np.array_equal(lb[:cap], want[2][:cap])
        assert (ei[cap:] == CANARY).all() and (lb[cap:] == CANARY).all()
    e.close()


def test_total_null_form_leaves_the_total_in_row_off():
    n_exprs, n_docs = 1000, 5000
    e = engine_with(n_exprs)
    bm = device_bitmap(n_docs, n_exprs, 0.01, seed=5)
    want = numpy_csr(bm, n_exprs)
    total = int(want[0][-1])
    ro, ei, _, t = compact(e, bm, n_docs, total, False, want_total=False)
    assert t is None and int(ro[n_docs]) == total
    assert np.array_equal(ro, want[0]) and np.array_equal(ei[:total], want[1])
    e.close()


def test_labels_belong_to_a_set_of_programs():
    e = engine_with(40, make_labels(40))
    bm = device_bitmap(8, 40, 0.5, seed=1)
    compact(e, bm, 8, 400, True)
    with pytest.raises(GftError) as ei:
        e.set_expr_labels(make_labels(39))                    # one label per expression
    assert ei.value.code == _lib.GFT_E_INVALID
    e.set_expr_labels(make_labels(40))
    e.set_programs([[1 << 28]] * 40)                          # any gft_set_programs clears the labels
    with pytest.raises(GftError) as ei:
        compact(e, bm, 8, 400, True)
    assert ei.value.code == _lib.GFT_E_INVALID
    ro, ei2, _, t = compact(e, bm, 8, 400, False)
    assert t == int(numpy_csr(bm, 40)[0][-1])
    e.set_expr_labels(make_labels(40))
    e.set_expr_labels(None)
    with pytest.raises(GftError):
        compact(e, bm, 8, 400, True)
    e.close()


def test_no_expressions_and_no_documents():
    e = engine_with(0)
    ro, _, _, t = compact(e, np.zeros((5, 0), np.uint32), 5, 0, False)
    assert t == 0 and not ro.any() and ro.shape == (6,)
    e.close()
    e = engine_with(70)
    ro, _, _, t = compact(e, np.zeros((0, 3), np.uint32), 0, 0, False)
    assert t == 0 and ro.tolist() == [0]
    e.close()


def test_a_handle_over_several_devices_is_refused():
    devs = [0, 1] if torch.cuda.device_count() >= 2 else [0, 0]
    e = Engine(devices=devs)
    e.build([b"aa", b"bb"])
    e.set_programs([[1 << 28]] * 40)
    bm = device_bitmap(8, 40, 0.5, seed=1)
    with pytest.raises(GftError) as ei:
        compact(e, bm, 8, 400, False)
    assert ei.value.code == _lib.GFT_E_UNSUPPORTED
    # the host-memory entry point serves such a handle through the host's compaction
    blob, off = pack_strings(["aa", "xx", "bb aa"])
    ro, idx, lb = e.process_sparse(blob, off)
    assert ro.tolist() == [0, 40, 40, 80] and lb is None and idx.tolist() == list(range(40)) * 2
    e.close()


# ---- the finder: fixtures of the reference -------------------------------------------------------------------------------
def _lists(ro, ei):
    ro, ei = ro.tolist(), ei.tolist()
    return [ei[ro[d]:ro[d + 1]] for d in range(len(ro) - 1)]


def _bitmap_lists(bm, n_exprs):
    return [[i for i in range(n_exprs) if row[i >> 5] >> (i & 31) & 1] for row in bm.tolist()]


@pytest.mark.parametrize("case", [c for c in load_golden("process_text.json")["cases"] if not c["expectedErr"]],
                         ids=lambda c: c["message"])
def test_results_of_a_batch_of_one_equal_process_text(case):
    text = load_golden("process_text.json")["text"]
    f, _, _ = make_mocked_finder(case, allow_no_device=False)
    got = f.ProcessTextsResults([text])
    assert len(got) == 1
    assert [r.to_obj() for r in got[0]] == case["expected"]
    f2, _, _ = make_mocked_finder(case, allow_no_device=False)
    assert [r.to_obj() for r in f2.ProcessText(text)] == [r.to_obj() for r in got[0]]


@pytest.mark.parametrize("case", [c for c in load_golden("process_text.json")["cases"] if c["expectedErr"]],
                         ids=lambda c: c["message"])
def test_sparse_batch_propagates_engine_errors(case):
    f, _, _ = make_mocked_finder(case, allow_no_device=False)
    with pytest.raises(FinderError) as ei:
        f.ProcessTextsSparse([load_golden("process_text.json")["text"]])
    assert str(ei.value) == case["expectedErr"]


@pytest.mark.parametrize("which", ["case_sensitive", "case_insensitive"])
def test_examples_as_one_batch(which):
    g = load_golden("examples.json")
    sec = g[which]
    f = Finder(GpuEngine(), PyRegexpEngine(), which == "case_sensitive")
    for e, tag in sec["expressions"]:
        f.AddExpressionWithTag(e, tag)
    ro, ei, tg = f.ProcessTextsSparse(g["texts"])
    assert _lists(ro, ei) == sec["expected_true"]
    tags = f.tags()
    assert [tags[t] for t in tg.tolist()] == [sec["expressions"][i][1] for i in ei.tolist()]
    res = f.ProcessTextsResults(g["texts"])
    for d, want in enumerate(sec["expected_true"]):
        assert [r.ExpresionIndex for r in res[d]] == want
        assert [r.Tag for r in res[d]] == [sec["expressions"][i][1] for i in want]
        assert [r.ExpresionStr for r in res[d]] == [sec["expressions"][i][0] for i in want]


# ---- the finder against the oracle -----------------------------------------------------------------------------------------
TAGS = ["alpha", "", "beta", "alpha", "gamma", ""]


def _tagged_finder(exprs, rgx=None, case_sensitive=False):
    """expressions registered in runs of 37 under TAGS in turn (repeated and empty tags)"""
    f = Finder(GpuEngine(), rgx or EmptyRgxEngine(), case_sensitive)
    want_tags = []
    for k in range(0, len(exprs), 37):
        tag = TAGS[(k // 37) % len(TAGS)]
        f.AddExpressionsWithTag(exprs[k:k + 37], tag)
        want_tags += [tag] * len(exprs[k:k + 37])
    return f, want_tags


def _check_sparse(f, want_tags, got, want_bm, n_exprs):
    ro, ei, tg = got
    want = _bitmap_lists(want_bm, n_exprs)
    assert ro.dtype == np.uint64 and ei.dtype == np.uint32 and tg.dtype == np.uint32
    assert _lists(ro, ei) == want
    tags = f.tags()
    assert [tags[t] for t in tg.tolist()] == [want_tags[i] for i in ei.tolist()]


def test_workload_corpus_equals_the_oracle():
    w = Workload(2000)
    exprs = make_expressions(w.terms(), 300, inord_fraction=0.3, cover=True)
    f, want_tags = _tagged_finder(exprs)
    o = Oracle(sorted(f.GetKeywords()))
    o.set_expressions(exprs, False)
    text, off = w.docs_host(0, 4000)
    want = o.process(text, off, fold=True)
    assert want.any()
    _check_sparse(f, want_tags, f.ProcessTextsSparse(blob=text, doc_off=off), want, len(exprs))
    assert _lib.load().gft_n_host_exprs(f.engine_handle()) == 0            # (the device route)
    res = f.ProcessTextsResults(blob=text, doc_off=off)
    assert [[r.ExpresionIndex for r in doc] for doc in res] == _bitmap_lists(want, len(exprs))
    assert all(r.Tag == want_tags[r.ExpresionIndex] and r.ExpresionStr == exprs[r.ExpresionIndex] for doc in res for r in doc)
    # an empty batch
    ro, ei, tg = f.ProcessTextsSparse([])
    assert ro.tolist() == [0] and ei.size == 0 and tg.size == 0
    f.close()


@pytest.mark.parametrize("prefilter", ["1", "0"])
def test_regex_terms_take_the_host_route(prefilter, monkeypatch):
    monkeypatch.setenv("GFT_REGEX_PREFILTER", prefilter)
    w = Workload(300)
    rx = ["en.*nr", "po[a-z]+ud", "q+"]
    exprs = make_expressions(w.terms(), 120, inord_fraction=0.4, regexes=rx)
    f, want_tags = _tagged_finder(exprs, PyRegexpEngine())
    text, off = w.docs_host(0, 200)
    o = Oracle(sorted(f.GetKeywords()))
    o.set_expressions(exprs, False)
    eng = PyRegexpEngine()
    eng.BuildEngine(sorted(f.GetRegexes()), False)
    offs, lits, poss = [0], [], []
    for d in range(200):
        for m in eng.FindRegexes(bytes(text[int(off[d]):int(off[d + 1])])):
            lits.append(o.literals.index(m.Term))
            poss.append(m.Position)
        offs.append(len(lits))
    assert lits
    extra = (np.asarray(offs, np.uint64), np.asarray(lits, np.int32), np.asarray(poss, np.int64))
    want = o.process(text, off, fold=True, extra=extra)
    _check_sparse(f, want_tags, f.ProcessTextsSparse(blob=text, doc_off=off), want, len(exprs))
    assert np.array_equal(f.ProcessTexts(blob=text, doc_off=off), want)
    f.close()


def test_a_host_solved_expression_takes_the_host_route():
    w = Workload(2000)
    terms = [t.decode() for t in w.terms()]
    exprs = make_expressions(w.terms(), 200, inord_fraction=0.3, cover=True)
    huge = "inord((%s) and (%s))" % (" or ".join('"%s"' % terms[i % 700] for i in range(4500)),
                                     " or ".join('"%s"' % terms[700 + i % 700] for i in range(4500)))
    exprs = exprs[:100] + [huge] + exprs[100:]
    f, want_tags = _tagged_finder(exprs)
    o = Oracle(sorted(f.GetKeywords()))
    o.set_expressions(exprs, False)
    text, off = w.docs_host(0, 300)
    want = o.process(text, off, fold=True)
    assert (want[:, 100 >> 5] >> (100 & 31) & 1).any()
    _check_sparse(f, want_tags, f.ProcessTextsSparse(blob=text, doc_off=off), want, len(exprs))
    assert _lib.load().gft_n_host_exprs(f.engine_handle()) == 1
    f.close()


def test_non_ascii_upper_case_batch_equals_the_oracle_after_tolower():
    exprs = ['"élan"', '"straße" and "ärger"', '"ωmega" or "zzz"', 'inord("ärger" and "élan")', '"ascii"', 'not "élan"']
    f, want_tags = _tagged_finder(exprs)
    texts = ["ÉLAN vital", "STRAßE und ÄRGER", "ΩMEGA", "ÄRGER vor ÉLAN", "ÉLAN vor ÄRGER", "plain ASCII text", ""] * 3
    o = Oracle(sorted(f.GetKeywords()))
    o.set_expressions(exprs, False)
    blob, off = pack_strings([t.lower() for t in texts])       # strings.ToLower of these texts is Python's lower()
    want = o.process(blob, off, fold=False)
    assert want[0, 0] & 1 and want[1, 0] >> 1 & 1 and want[2, 0] >> 2 & 1 and want[3, 0] >> 3 & 1 and not want[4, 0] >> 3 & 1
    _check_sparse(f, want_tags, f.ProcessTextsSparse(texts), want, len(exprs))
    # a large batch goes up unchecked and comes back for the host's ToLower (gft_last_nonascii)
    unit = texts + ["plain ascii filler " * 200]
    many = unit * 4500
    assert sum(len(t.encode()) for t in many) >= 16 << 20
    blob, off = pack_strings([t.lower() for t in unit])
    one = _bitmap_lists(o.process(blob, off, fold=False), len(exprs))
    ro, ei, tg = f.ProcessTextsSparse(many)
    assert _lists(ro, ei) == one * 4500
    f.close()


def _device_batch(blob, off):
    t = torch.from_numpy(np.concatenate([blob, np.zeros(64, np.uint8)])).cuda()
    o = torch.from_numpy(off.astype(np.int64)).cuda()
    return t, o


def test_compaction_of_batch_a_while_batch_b_is_in_flight():
    w = Workload(2000)
    exprs = make_expressions(w.terms(), 300, inord_fraction=0.3, cover=True)
    f, want_tags = _tagged_finder(exprs)
    o = Oracle(sorted(f.GetKeywords()))
    o.set_expressions(exprs, False)
    words = (len(exprs) + 31) // 32
    batches = []
    for k, n in enumerate((3000, 2500)):
        text, off = w.docs_host(k * 3000, n)
        off = off - off[0]
        t, od = _device_batch(text, off)
        batches.append(dict(n=n, t=t, o=od, want=o.process(text, off, fold=True),
                            bm=torch.zeros((n, words), dtype=torch.int32, device="cuda")))
    A, B = batches
    for _ in range(4):                                           # sizes learnt: the next batches run deferred
        f.ProcessDevice(A["t"].data_ptr(), A["o"].data_ptr(), A["n"], A["bm"].data_ptr())
    A["bm"].zero_()
    cap = 1 << 20
    out = {}
    for name, b in (("A", A), ("B", B)):
        out[name] = (torch.full((b["n"] + 1,), -1, dtype=torch.int64, device="cuda"),
                     torch.zeros(cap, dtype=torch.int32, device="cuda"), torch.zeros(cap, dtype=torch.int32, device="cuda"))
    f.ProcessDeviceBegin(A["t"].data_ptr(), A["o"].data_ptr(), A["n"], A["bm"].data_ptr())
    f.ProcessDeviceBegin(B["t"].data_ptr(), B["o"].data_ptr(), B["n"], B["bm"].data_ptr())
    f.ProcessDeviceEnd()
    # with a younger batch in flight the waiting form is refused, the enqueue-only form is the one to use
    assert f.CompactDevice(A["bm"].data_ptr(), A["n"], *(x.data_ptr() for x in out["A"]), cap, want_total=False) is None
    f.ProcessDeviceEnd()
    total_b = f.CompactDevice(B["bm"].data_ptr(), B["n"], *(x.data_ptr() for x in out["B"]), cap)
    torch.cuda.synchronize()
    for name, b in (("A", A), ("B", B)):
        ro, ei, tg = (x.cpu().numpy() for x in out[name])
        ro = ro.astype(np.uint64)
        total = int(ro[b["n"]])
        assert 0 < total <= cap
        if name == "B":
            assert total == total_b
        _check_sparse(f, want_tags, (ro, ei.view(np.uint32)[:total], tg.view(np.uint32)[:total]), b["want"], len(exprs))
        assert np.array_equal(b["bm"].cpu().numpy().view(np.uint32), b["want"])         # the bitmaps are as the solver left them
    f.close()


def test_waiting_form_is_refused_while_a_batch_is_in_flight():
    w = Workload(2000)
    exprs = make_expressions(w.terms(), 100, cover=True)
    f, _ = _tagged_finder(exprs)
    words = (len(exprs) + 31) // 32
    text, off = w.docs_host(0, 2000)
    t, od = _device_batch(text, off)
    bm = torch.zeros((2000, words), dtype=torch.int32, device="cuda")
    for _ in range(4):
        f.ProcessDevice(t.data_ptr(), od.data_ptr(), 2000, bm.data_ptr())
    ro = torch.zeros(2001, dtype=torch.int64, device="cuda")
    f.ProcessDeviceBegin(t.data_ptr(), od.data_ptr(), 2000, bm.data_ptr())
    L = _lib.load()
    total = C.c_uint64()
    rc = L.gft_compact_device(f.engine_handle(), bm.data_ptr(), 2000, ro.data_ptr(), None, None, 0, C.byref(total))
    assert rc == _lib.GFT_E_INVALID                             # (it would have to wait for the stream)
    f.ProcessDeviceEnd()
    assert f.CompactDevice(bm.data_ptr(), 2000, ro.data_ptr(), None, None, 0) == int(ro[2000].item())
    f.close()
