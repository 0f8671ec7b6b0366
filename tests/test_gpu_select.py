"""The documents that matched, gathered into one blob on the device (csrc/gft_select.hip): Engine.select_docs_device and the raw
C call against the reference of select_docs.py AND the host walk on every fixed and random case, with the text and the output at
every kind of residue of the 16-byte grid and the slack filled two ways; the cap protocol into guarded tensors; the refusals; one
batch whose output passes 4 GiB; and the callers -- Finder.SelectLinesDevice / SelectLines against ProcessTexts over the pieces,
GroupFinder.SelectJsonLinesDevice / SelectJsonLines against ProcessJsons over the lines.  All comparisons are exact."""
import ctypes as C
import functools
import json

import numpy as np
import pytest
import torch  # noqa: F401  (before libgft.so is loaded: one HIP runtime)

import far_text as F
import json_docs as J
import select_docs as S
import split_lines as SL
from gofindthem_amd import _lib, group
from gofindthem_amd.engine import Engine, GftError, select_docs_host, _want_words
from gofindthem_amd.finder import EmptyRgxEngine, Finder, FinderError, GpuEngine, PyRegexpEngine
from gofindthem_amd.workload import Workload

pytestmark = pytest.mark.gpu

GUARD8, GUARD64 = 0xA5, -0x5A5A5A5A5A5A5A5B
OFFSETS = (0, 1, 3, 8, 15)


@pytest.fixture(scope="module")
def eng():
    e = Engine()
    yield e
    e.close()


def resident(blob, at=0, fill=0):
    """the blob at byte `at` of an allocation whose other bytes -- the 64 of slack among them -- hold `fill`"""
    blob = bytes(blob)
    buf = torch.full((at + len(blob) + 64 + 16,), fill, dtype=torch.uint8, device="cuda")
    if blob:
        buf[at:at + len(blob)] = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    return buf[at:]


class OnDevice:
    """a case of select_docs.py on the device, its text `at` bytes into its allocation"""

    def __init__(self, c, at=0, fill=0):
        self.c = c
        self.text = resident(c.blob.tobytes(), at, fill)
        self.off = torch.from_numpy(c.doc_off.astype(np.int64)).cuda()
        self.rows = torch.from_numpy(c.rows.view(np.int32).copy()).cuda()
        self.also = torch.from_numpy(c.also).cuda() if c.also is not None else None
        self.n = len(c.doc_off) - 1


@functools.lru_cache(maxsize=None)
def host_walk():
    """{name: (bytes, out_off, doc_idx)} of gft_debug_select_docs, computed once"""
    out = {}
    for c in S.all_cases():
        m, total, data, off, idx = select_docs_host(c.blob, c.doc_off, c.rows, c.n_cols, c.want, c.mode, c.also)
        out[c.name] = (data[:total].tobytes(), off[:m + 1].tolist(), idx[:m].tolist())
    return out


def raw_select(eng, d, cap_bytes=None, cap_docs=None, out_at=0, guard=32, mode=None):
    """gft_select_docs_device into guarded tensors, the output `out_at` bytes into its allocation -> (m, total, out, out_off,
    doc_idx) on the host, guards included.  Caps None: count first"""
    L = _lib.load()
    c = d.c
    W = (c.n_cols + 31) // 32
    w = _want_words(c.want, c.n_cols)
    head = (eng._h, d.text.data_ptr(), d.off.data_ptr(), d.n, d.rows.data_ptr() if W and d.n else None, c.n_cols, w.ctypes.data if w is not None else None,
            S.MODES[c.mode] if mode is None else mode, d.also.data_ptr() if d.also is not None else None)
    m, t = C.c_uint64(99), C.c_uint64(99)
    torch.cuda.synchronize()
    if cap_bytes is None:
        eng._check(L.gft_select_docs_device(*head, None, 0, None, None, 0, C.byref(m), C.byref(t)))
        cap_bytes, cap_docs = int(t.value), int(m.value)
    out = torch.full((out_at + cap_bytes + guard,), GUARD8, dtype=torch.uint8, device="cuda")
    oo = torch.full((cap_docs + 1 + guard,), GUARD64, dtype=torch.int64, device="cuda")
    di = torch.full((cap_docs + guard,), GUARD64, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    eng._check(L.gft_select_docs_device(*head, out.data_ptr() + out_at, cap_bytes, oo.data_ptr(), di.data_ptr(), cap_docs, C.byref(m), C.byref(t)))
    return int(m.value), int(t.value), out.cpu().numpy(), oo.cpu().numpy(), di.cpu().numpy()


def check_raw(eng, d, out_at):
    c = d.c
    data, off, idx = S.expected()[c.name]
    assert host_walk()[c.name] == (data, off, idx), c.name
    m, total, out, oo, di = raw_select(eng, d, out_at=out_at)
    assert (m, total) == (len(idx), len(data)), c.name
    assert (out[:out_at] == GUARD8).all() and out[out_at:out_at + total].tobytes() == data and (out[out_at + total:] == GUARD8).all(), (c.name, out_at)
    assert oo[:m + 1].tolist() == off and (oo[m + 1:] == GUARD64).all() and di[:m].tolist() == idx and (di[m:] == GUARD64).all(), (c.name, out_at)


def test_the_cases_are_not_vacuous():
    assert S.assert_not_vacuous()


def test_fixed_cases(eng):
    for c in S.fixed_cases():
        d = OnDevice(c)
        out, out_off, doc_idx = eng.select_docs_device(d.text, d.off, d.rows, c.n_cols, c.want, c.mode, d.also)
        data, off, idx = S.expected()[c.name]
        assert out.cpu().numpy().tobytes() == data and out_off.cpu().tolist() == off and doc_idx.cpu().tolist() == idx, c.name
        assert host_walk()[c.name] == (data, off, idx), c.name


@pytest.mark.parametrize("fill", [0, 0xFF], ids=["zeros behind", "ones behind"])
def test_text_and_output_at_every_residue_and_what_the_slack_holds(eng, fill):
    for c in S.fixed_cases():
        for at in OFFSETS:
            d = OnDevice(c, at, fill)
            out, out_off, doc_idx = eng.select_docs_device(d.text, d.off, d.rows, c.n_cols, c.want, c.mode, d.also)
            data, off, idx = S.expected()[c.name]
            assert out.cpu().numpy().tobytes() == data and out_off.cpu().tolist() == off and doc_idx.cpu().tolist() == idx, (c.name, at)
            check_raw(eng, d, OFFSETS[(OFFSETS.index(at) + 2) % 5])
        d = OnDevice(c, 0, fill)
        for out_at in OFFSETS:
            check_raw(eng, d, out_at)


@pytest.mark.parametrize("fill", [0, 0xFF], ids=["zeros behind", "ones behind"])
def test_random_batches(eng, fill):
    for c in S.random_cases():
        data, off, idx = S.expected()[c.name]
        for i, at in enumerate(OFFSETS):
            d = OnDevice(c, at, fill)
            out, out_off, doc_idx = eng.select_docs_device(d.text, d.off, d.rows, c.n_cols, c.want, c.mode, d.also)
            assert out.cpu().numpy().tobytes() == data and out_off.cpu().tolist() == off and doc_idx.cpu().tolist() == idx, (c.name, at)
            check_raw(eng, d, OFFSETS[(i + 2) % 5])
        d = OnDevice(c, 0, fill)
        for out_at in OFFSETS:
            check_raw(eng, d, out_at)


def test_cap_protocol(eng):
    c = next(c for c in S.fixed_cases() if c.name == "edge lengths, every other one")
    data, off, idx = S.expected()[c.name]
    total, m = len(data), len(idx)
    mid = (off[3] + off[4]) // 2
    assert off[3] < mid < off[4]
    d = OnDevice(c, 3)
    for out_at in (0, 5):
        for cb in (total, total - 1, mid, 1, 0):
            for cd in (m, m - 1, 1, 0):
                gm, gt, out, oo, di = raw_select(eng, d, cb, cd, out_at)
                assert (gm, gt) == (m, total), (cb, cd)
                k = min(m, cd)
                assert (out[:out_at] == GUARD8).all() and out[out_at:out_at + cb].tobytes() == data[:cb] and (out[out_at + cb:] == GUARD8).all(), (cb, cd)
                assert oo[:k + 1].tolist() == off[:k + 1] and (oo[k + 1:] == GUARD64).all(), (cb, cd)
                assert di[:k].tolist() == idx[:k] and (di[k:] == GUARD64).all(), (cb, cd)
    # a cap past the total: nothing behind the total is touched
    gm, gt, out, _, _ = raw_select(eng, d, total + 40, m, 7)
    assert out[7:7 + total].tobytes() == data and (out[7 + total:] == GUARD8).all()
    # count only, and no documents
    L = _lib.load()
    n_sel, n_bytes = C.c_uint64(9), C.c_uint64(9)
    oo = torch.full((4,), GUARD64, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert L.gft_select_docs_device(eng._h, None, None, 0, None, 5, None, 0, None, None, 0, oo.data_ptr(), None, 0, C.byref(n_sel), C.byref(n_bytes)) == 0
    assert (n_sel.value, n_bytes.value) == (0, 0) and oo.cpu().tolist() == [0] + [GUARD64] * 3


def test_refusals_leave_the_handle_usable(eng):
    L = _lib.load()
    E = _lib.GFT_E_INVALID
    c = next(c for c in S.fixed_cases() if c.name == "also, any")
    d = OnDevice(c)
    data, off, idx = S.expected()[c.name]
    W = (c.n_cols + 31) // 32
    out = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda")
    oo = torch.zeros(len(idx) + 1, dtype=torch.int64, device="cuda")
    di = torch.zeros(len(idx), dtype=torch.int64, device="cuda")
    m, t = C.c_uint64(0), C.c_uint64(0)
    torch.cuda.synchronize()

    def call(text=d.text.data_ptr(), doc_off=d.off.data_ptr(), mode=0, o=out.data_ptr(), cb=len(data), oop=oo.data_ptr(), dip=di.data_ptr(), cd=len(idx)):
        return L.gft_select_docs_device(eng._h, text, doc_off, d.n, d.rows.data_ptr(), c.n_cols, c.want.ctypes.data, mode, d.also.data_ptr(), o, cb, oop,
                                        dip, cd, C.byref(m), C.byref(t))
    assert call() == 0
    assert call(mode=3) == E                                                     # unknown mode
    assert L.gft_last_error(eng._h).decode() == "gft_select_docs_device: unknown mode"
    assert call(cd=1 << 61) == E                                                 # a size beyond the address space
    assert L.gft_last_error(eng._h).decode() == "gft_select_docs_device: a size beyond the address space"
    assert call(o=None) == E and call(oop=None) == E and call(dip=None) == E     # a cap without its array
    assert call(o=d.text.data_ptr() + int(c.doc_off[0]), cb=3) == E              # the output over the text ...
    assert call(o=d.off.data_ptr(), cb=3) == E                                   # ... the offsets ...
    assert call(o=d.rows.data_ptr() + 4 * W * (d.n - 1), cb=3) == E              # ... the last row ...
    assert call(o=d.also.data_ptr() + d.n - 1, cb=1) == E                        # ... the last byte of `also`
    assert call(oop=d.rows.data_ptr()) == E and call(dip=d.off.data_ptr()) == E
    assert "overlaps" in L.gft_last_error(eng._h).decode()
    assert L.gft_last_error(eng._h).decode() == "gft_select_docs_device: an output overlaps an input"
    down = d.off.clone()
    down[3], down[4] = d.off[4].item(), d.off[3].item()
    if down[3] == down[4]:
        down[4] -= 1
    torch.cuda.synchronize()
    assert call(doc_off=down.data_ptr()) == E                                    # offsets that descend
    assert "descend" in L.gft_last_error(eng._h).decode()
    assert L.gft_last_error(eng._h).decode() == "gft_select_docs_device: document offsets descend, or a document of 4 GiB or more"
    huge = d.off.clone()
    huge[d.n] += 1 << 32
    torch.cuda.synchronize()
    assert call(doc_off=huge.data_ptr(), o=None, cb=0, oop=None, dip=None, cd=0) == E      # a document of 4 GiB or more
    assert L.gft_last_error(eng._h).decode() == "gft_select_docs_device: document offsets descend, or a document of 4 GiB or more"
    with pytest.raises(ValueError):
        eng.select_docs_device(d.text, d.off, d.rows, c.n_cols, np.zeros(W + 1, np.uint32))
    got = eng.select_docs_device(d.text, d.off, d.rows, c.n_cols, c.want, c.mode, d.also)
    assert got[0].cpu().numpy().tobytes() == data and got[2].cpu().tolist() == idx


def test_profile_names_and_the_verdict_is_left_alone(eng):
    L = _lib.load()
    before = L.gft_last_nonascii(eng._h)
    c = S.random_cases()[2]
    d = OnDevice(c)
    eng.profile(True)
    eng.profile_reset()
    eng.select_docs_device(d.text, d.off, d.rows, c.n_cols, c.want, c.mode, d.also)
    counts = {name: eng.profile_read(name)[1] for name in ("select_mark", "select_scan", "select_place", "select_copy")}
    eng.profile(False)
    assert counts == {"select_mark": 2, "select_scan": 2, "select_place": 2, "select_copy": 1}     # (count only, then the fill)
    assert L.gft_last_nonascii(eng._h) == before


def test_handles_over_several_devices_are_refused():
    c = S.fixed_cases()[0]
    d = OnDevice(c)
    e = Engine(devices=[0, 0])
    with pytest.raises(GftError) as ei:
        e.select_docs_device(d.text, d.off, d.rows, c.n_cols, c.want, c.mode)
    assert ei.value.code == _lib.GFT_E_UNSUPPORTED
    e.close()
    one = Engine()
    assert one.select_docs_device(d.text, d.off, d.rows, c.n_cols, c.want, c.mode)[2].cpu().tolist() == S.expected()[c.name][2]
    one.close()


def test_an_output_past_four_gib(eng):
    """70 documents of 64 MiB, all but three selected: the output positions pass 2^32, the one place a 32-bit offset would hide.
    Every byte is the top byte of its 64-bit position times far_text.GOLDEN, which depends on every bit of the position: no two
    documents, and no two positions 2^32 apart, hold the same bytes (the ramp this replaces repeated every 2 MiB, so every
    document held the same bytes and the copy of a wrong document, or from a source position cut to 32 bits, passed)"""
    n, size = 70, 64 << 20
    text = torch.empty(n * size + 64, dtype=torch.uint8, device="cuda")
    ramp = torch.arange(size, dtype=torch.int64, device="cuda")
    for k in range(n):
        text[k * size:(k + 1) * size] = F.top_byte_torch(ramp + k * size).to(torch.uint8)
    del ramp
    assert text[(1 << 32) - 512:(1 << 32) + 512].cpu().numpy().tobytes() == F.top_byte(np.arange((1 << 32) - 512, (1 << 32) + 512)).tobytes()
    off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * size
    rows = torch.full((n, 1), -2, dtype=torch.int32, device="cuda")                 # column 0 clear, the tail bits ones
    keep = [k for k in range(n) if k not in (0, 35, 69)]
    rows[keep, 0] = -1
    # two different source documents differ in their first KiB, and so do positions 2^32 apart (with the old ramp neither held)
    for a in range(n - 1):
        assert not torch.equal(text[a * size:a * size + 1024], text[(a + 1) * size:(a + 1) * size + 1024]), a
    assert not torch.equal(text[:1024], text[35 * size:35 * size + 1024]) and not torch.equal(text[size:size + 1024], text[65 * size:65 * size + 1024])
    out, out_off, doc_idx = eng.select_docs_device(text, off, rows, 1, None, "any")
    assert doc_idx.cpu().tolist() == keep and out_off.cpu().tolist() == [k * size for k in range(len(keep) + 1)]
    assert out.numel() == len(keep) * size > 1 << 32
    for k, src in enumerate(keep):
        a, b = k * size, src * size
        assert torch.equal(out[a:a + 1024], text[b:b + 1024]) and torch.equal(out[a + size - 1024:a + size], text[b + size - 1024:b + size]), k
        assert torch.equal(out[a:a + size], text[b:b + size]), k
    del out, text
    torch.cuda.empty_cache()


# ---- the finder -----------------------------------------------------------------------------------------------------------------
def lines_finder(n=3000):
    w = Workload(n)
    text, off = w.docs_host(0, n)
    docs = [bytes(text[int(off[i]):int(off[i + 1])]).replace(b"\n", b" ") for i in range(n)]
    terms = [t.decode("ascii") for t in w.terms() if t.isalpha()][:40]
    docs[7] = b""                                                      # an empty line
    docs[20] = ("VIVE LA École " + terms[1].upper()).encode("utf-8")   # leaves ASCII: lowered on the device, scanned again
    blob = b"\n".join(docs) + b"\n"
    f = Finder(GpuEngine(), EmptyRgxEngine(), False)
    for i, t in enumerate(terms[:20]):
        f.AddExpressionWithTag('"%s"' % t, "tag%d" % (i % 3))
    f.AddExpressionWithTag('"école" and "%s"' % terms[1], "french")
    f.AddExpressionWithTag('"%s" and not "%s"' % (terms[2], terms[3]), "tag0")
    return f, blob, SL.documents(blob, SL.AFTER_NL)


def test_finder_select_lines():
    f, blob, pieces = lines_finder()
    assert len(pieces) == 3000 and pieces[7] == b"\n"
    rows = f.ProcessTexts(pieces)
    off = SL.reference(blob, SL.AFTER_NL)
    E = f.n_expressions
    masks = [(None, "any"), (f.want_mask(indices=[0, 5]), "any"), (f.want_mask(tags=["french"]), "any"), (f.want_mask(tags=["tag1", "french"]), "none"),
             (f.want_mask(indices=[2, 3]), "all")]
    before = f.lowered_batches()
    for want, mode in masks:
        data, out_off, idx = S.reference(blob, off, rows, E, want, mode, None)
        assert len(idx) < 3000 and (idx or mode == "all"), mode
        out, d_out_off, d_idx, d_off, d_rows = f.SelectLinesDevice(resident(blob, 3), len(blob), want, mode)
        assert out.cpu().numpy().tobytes() == data and d_out_off.cpu().tolist() == out_off and d_idx.cpu().tolist() == idx, mode
        assert d_off.cpu().tolist() == off and np.array_equal(d_rows.cpu().numpy().view(np.uint32), rows)
        h = f.SelectLines(blob, want, mode)
        assert h[0] == data and h[1].tolist() == out_off and h[2].tolist() == idx, mode
    assert f.lowered_batches() == (before[0] + 2 * len(masks), before[1])           # the lowering repeat ran every time
    assert 20 in S.reference(blob, off, rows, E, f.want_mask(tags=["french"]), "any", None)[2]
    data, out_off, idx = f.SelectLines(b"")
    assert data == b"" and out_off.tolist() == [0] and idx.tolist() == []
    f.close()


def test_finder_select_needs_what_process_device_needs_and_selects_on_the_host_then():
    f = Finder(GpuEngine(), PyRegexpEngine(), False)
    f.AddExpressions(['"ab"', 'r"c+d"'])
    buf = resident(b"ab\ncd\nxx\n")
    off = torch.tensor([0, 3, 6, 9], dtype=torch.int64, device="cuda")
    rows = torch.zeros((3, 1), dtype=torch.int32, device="cuda")
    with pytest.raises(FinderError) as e1:
        f.SelectDevice(buf, off, rows)
    with pytest.raises(FinderError) as e2:
        f.ProcessDevice(buf.data_ptr(), off.data_ptr(), 3, rows.data_ptr())
    assert e1.value.code == e2.value.code == _lib.GFT_E_UNSUPPORTED and str(e1.value) == str(e2.value)
    # the host-memory form goes on answering: rows from ProcessTexts, the select by the kernels' walk on the host
    data, out_off, idx = f.SelectLines(b"ab\ncd\nxx\nccd ab\n")
    assert data == b"ab\ncd\nccd ab\n" and out_off.tolist() == [0, 3, 6, 13] and idx.tolist() == [0, 1, 3]
    data, _, idx = f.SelectLines(b"ab\ncd\nxx\nccd ab\n", f.want_mask(indices=[1]), "none")
    assert data == b"ab\nxx\n" and idx.tolist() == [0, 2]
    f.close()


def test_select_between_begin_and_end_only_after_complete():
    f, blob, pieces = lines_finder(2000)
    L = _lib.load()
    eh = f.engine_handle()
    buf = resident(blob)
    off = f.SplitLinesDevice(buf, len(blob), 0)
    n = off.numel() - 1
    W = (f.n_expressions + 31) // 32
    bm = torch.zeros((n, W), dtype=torch.int32, device="cuda")
    for _ in range(4):                                                   # sizes learnt: the next batch runs deferred
        f.ProcessDevice(buf.data_ptr(), off.data_ptr(), n, bm.data_ptr())
    rows = bm.clone()
    want = f.want_mask(indices=[1, 4])
    data, out_off, idx = S.reference(blob, off.cpu().tolist(), rows.cpu().numpy().view(np.uint32), f.n_expressions, want, "any", None)
    assert 0 < len(idx) < n
    m, t = C.c_uint64(0), C.c_uint64(0)
    args = (buf.data_ptr(), off.data_ptr(), n, rows.data_ptr(), f.n_expressions, want.ctypes.data, 0, None, None, 0, None, None, 0, C.byref(m), C.byref(t))
    torch.cuda.synchronize()
    f.ProcessDeviceBegin(buf.data_ptr(), off.data_ptr(), n, bm.data_ptr())
    assert L.gft_select_docs_device(eh, *args) == _lib.GFT_E_INVALID
    assert "in flight" in L.gft_last_error(eh).decode()
    with pytest.raises(FinderError):
        f.SelectDevice(buf, off, rows, want)                             # the finder's form waits for ProcessDeviceEnd
    assert L.gft_process_device_complete(eh) == 0
    assert L.gft_select_docs_device(eh, *args) == 0 and (m.value, t.value) == (len(idx), len(data))
    f.ProcessDeviceEnd()
    assert torch.equal(bm, rows)
    out, d_out_off, d_idx = f.SelectDevice(buf, off, rows, want)
    assert out.cpu().numpy().tobytes() == data and d_idx.cpu().tolist() == idx and d_out_off.cpu().tolist() == out_off
    f.close()


# ---- the group finder -------------------------------------------------------------------------------------------------------------
TABLE_EXPRS = ['"x"', '"y"', '"v"', '"lorem" and "ipsum"', '"p"', '"s" or "q"', '"first"', 'inord("lorem" and "ipsum")', '"é"', '"w"']
TABLE_TAGS = ["t0", "t1", "t0", "t2", "t1", "t2", "t0", "t3", "t3", "t1"]
TABLE_RULES = {"any x": ['"t0"', '"t0:a"', 'not "t1"'], 'quo"te': ['"t2" or "t3:m.n"', 'not "t0:k"'], "z\\last": ['"t1" and not "t2"']}
WS = b" \t\r\n"


def table_group():
    f = Finder(GpuEngine(), EmptyRgxEngine(), False)
    for e, t in zip(TABLE_EXPRS, TABLE_TAGS):
        f.AddExpressionWithTag(e, t)
    g = group.NewFinderWithRules(f, TABLE_RULES)
    g.SetSchema(J.SCHEMA)
    return g


def table_lines():
    """the table's documents that fit a line, a line each, with a mix of line ends and indentation"""
    raws = [d for d in J.table() if d.schema is J.SCHEMA and b"\n" not in d.raw and d.raw.strip(WS) and len(d.raw) < 5000]
    ends = [b"\n", b"\r\n", b"\n\n", b"\n \t\r\n"]
    blob = b"".join((b"  " if i % 5 == 0 else b"") + d.raw + ends[i % 4] for i, d in enumerate(raws))
    lines = SL.documents(blob, SL.JSON_LINES)
    assert len(lines) == len(raws) and b"".join(lines) == blob
    return blob, lines, raws


@pytest.mark.parametrize("keep_undecided", [True, False])
def test_select_json_lines_device(keep_undecided):
    g = table_group()
    blob, lines, docs = table_lines()
    off = SL.reference(blob, SL.JSON_LINES)
    buf = resident(blob, 1, ord("{"))
    _, d_rows, d_status = g.ProcessJsonLinesDevice(buf, len(blob))
    rows, status = d_rows.cpu().numpy().view(np.uint32), d_status.cpu().numpy()
    assert set(status.tolist()) == {J.OK, J.SYNTAX, J.DEPTH, J.PATH, J.KEY, J.DUP, J.TEXT}        # every status
    assert status.tolist() == g.ProcessJsonsDevice(*J.to_device(lines))[1].cpu().tolist()
    results = g.ProcessJsons(lines)
    n_cols = len(g.rule_exprs())
    sizes = set()
    for rules, mode in ((None, "any"), (["any x"], "any"), (['quo"te', "z\\last"], "any"), (["any x"], "none"), (['quo"te'], "all")):
        out, out_off, doc_idx, st = g.SelectJsonLinesDevice(buf, len(blob), rules, mode, keep_undecided)
        assert torch.equal(st.cpu(), d_status.cpu())
        data, want_off, idx = S.reference(blob, off, rows, n_cols, g.rule_mask(rules), mode, status if keep_undecided else None)
        assert out.cpu().numpy().tobytes() == data and out_off.cpu().tolist() == want_off and doc_idx.cpu().tolist() == idx, (rules, mode)
        picked = set(idx)
        names = set(r for r, _ in g.rule_exprs()) if rules is None else set(rules)
        for i, r in enumerate(results):
            if status[i] != 0:
                assert not keep_undecided or i in picked, i
            elif mode == "any":
                assert (i in picked) == bool(names & set(r.get("rules", {}))), (i, rules)
            elif mode == "none":
                assert (i in picked) == (not names & set(r.get("rules", {}))), (i, rules)
        sizes.add(len([i for i in idx if status[i] == 0]))
        if keep_undecided:
            assert {i for i in range(len(docs)) if status[i] != 0} <= picked
    assert len(sizes) > 2 and 0 < min(sizes) and max(sizes) <= int((status == 0).sum())


def test_select_json_lines():
    g = table_group()
    blob, lines, docs = table_lines()
    results = g.ProcessJsons(lines)
    status = g.ProcessJsonsDevice(*J.to_device(lines))[1].cpu().tolist()
    data, out_off, doc_idx, undecided = g.SelectJsonLines(blob, ["any x"], "any")
    assert undecided.tolist() == [i for i, s in enumerate(status) if s != 0] and set(undecided.tolist()) <= set(doc_idx.tolist()) and len(undecided) > 10
    assert data == b"".join(lines[i] for i in doc_idx.tolist())
    assert [int(out_off[k + 1] - out_off[k]) for k in range(len(doc_idx))] == [len(lines[i]) for i in doc_idx.tolist()]
    decided = [i for i in doc_idx.tolist() if status[i] == 0]
    assert decided == [i for i, r in enumerate(results) if status[i] == 0 and "any x" in r.get("rules", {})] and decided
    # the output is JSON Lines again: every decided line parses, and the split finds the same documents
    again = SL.documents(data, SL.JSON_LINES)
    assert again == [lines[i] for i in doc_idx.tolist()]
    for k, i in enumerate(doc_idx.tolist()):
        if status[i] == 0:
            json.loads(again[k].decode("utf-8"))
    with pytest.raises(ValueError):
        g.SelectJsonLines(blob, ["no such rule"])
