"""Context lines round the documents that matched, on the device (csrc/gft_context.hip): Engine.context_docs_device and the raw C
call against the reference of context_docs.py AND the host walk on every fixed and random case, into guarded tensors, with the
text and the output at two residues of the 16-byte grid each; the three caps; count only; the refusals; the identity with the
select; one batch whose text lies past 4 GiB; and Finder.ContextLinesDevice / ContextLines against ProcessTexts over the pieces.
All comparisons are exact."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (before libgft.so is loaded: one HIP runtime)

import context_docs as X
import far_text as F
import select_docs as S
import split_lines as SL
from gofindthem_amd import _lib
from gofindthem_amd.engine import Engine, GftError, context_docs_host, _want_words
from gofindthem_amd.finder import EmptyRgxEngine, Finder, FinderError, GpuEngine
from gofindthem_amd.workload import Workload

pytestmark = pytest.mark.gpu

GUARD8, GUARD64 = 0xA5, -0x5A5A5A5A5A5A5A5B
RESIDUES = ((0, 0), (5, 11), (8, 3))                                # (text at, output at): two residues each beside the aligned one
FRONT = 16                                                          # guard entries in front of every output


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
    """a case of context_docs.py (or of select_docs.py: no reach, no fence) on the device, its text `at` bytes into its allocation"""

    def __init__(self, c, at=0, fill=0):
        self.c = c
        self.text = resident(c.blob.tobytes(), at, fill)
        self.off = torch.from_numpy(c.doc_off.astype(np.int64)).cuda()
        self.rows = torch.from_numpy(c.rows.view(np.int32).copy()).cuda()
        self.also = torch.from_numpy(c.also).cuda() if c.also is not None else None
        fence = getattr(c, "fence", None)
        self.fence = torch.from_numpy(fence).cuda() if fence is not None else None
        self.before, self.after = getattr(c, "before", 0), getattr(c, "after", 0)
        self.n = len(c.doc_off) - 1

    def call(self, eng):
        c = self.c
        return eng.context_docs_device(self.text, self.off, self.rows, c.n_cols, c.want, c.mode, self.also, self.before, self.after, self.fence)


def on_host(r):
    out, out_off, doc_idx, kind, group_off = r
    return out.cpu().numpy().tobytes(), out_off.cpu().tolist(), doc_idx.cpu().tolist(), kind.cpu().tolist(), group_off.cpu().tolist()


@functools.lru_cache(maxsize=None)
def host_walk():
    """{name: (bytes, out_off, doc_idx, kind, group_off)} of gft_debug_context_docs, computed once"""
    out = {}
    for c in X.all_cases():
        m, _, g, total, data, off, idx, kind, go = context_docs_host(c.blob, c.doc_off, c.rows, c.n_cols, c.want, c.mode, c.also, c.before, c.after, c.fence)
        out[c.name] = (data[:total].tobytes(), off[:m + 1].tolist(), idx[:m].tolist(), kind[:m].tolist(), go[:g + 1].tolist())
    return out


def raw_context(eng, d, cap_bytes=None, cap_docs=None, cap_groups=None, out_at=0, guard=32, mode=None):
    """gft_context_docs_device into guarded tensors -- FRONT entries in front of every output, `guard` behind --, the bytes `out_at`
    further into their allocation -> (counts, out, out_off, doc_idx, kind, group_off) on the host, guards included.  Caps None:
    count first"""
    L = _lib.load()
    c = d.c
    W = (c.n_cols + 31) // 32
    w = _want_words(c.want, c.n_cols)
    head = (eng._h, d.text.data_ptr(), d.off.data_ptr(), d.n, d.rows.data_ptr() if W and d.n else None, c.n_cols, w.ctypes.data if w is not None else None,
            S.MODES[c.mode] if mode is None else mode, d.also.data_ptr() if d.also is not None else None, int(d.before), int(d.after),
            d.fence.data_ptr() if d.fence is not None else None)
    cnt = [C.c_uint64(99) for _ in range(4)]
    refs = [C.byref(x) for x in cnt]
    torch.cuda.synchronize()
    if cap_bytes is None:
        eng._check(L.gft_context_docs_device(*head, None, 0, None, None, None, 0, None, 0, *refs))
        cap_docs, _, cap_groups, cap_bytes = (int(x.value) for x in cnt)
    lead = FRONT + out_at
    out = torch.full((lead + cap_bytes + guard,), GUARD8, dtype=torch.uint8, device="cuda")
    oo = torch.full((FRONT + cap_docs + 1 + guard,), GUARD64, dtype=torch.int64, device="cuda")
    di = torch.full((FRONT + cap_docs + guard,), GUARD64, dtype=torch.int64, device="cuda")
    ki = torch.full((FRONT + cap_docs + guard,), GUARD8, dtype=torch.uint8, device="cuda")
    go = torch.full((FRONT + cap_groups + 1 + guard,), GUARD64, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    eng._check(L.gft_context_docs_device(*head, out.data_ptr() + lead, cap_bytes, oo.data_ptr() + 8 * FRONT, di.data_ptr() + 8 * FRONT,
                                         ki.data_ptr() + FRONT, cap_docs, go.data_ptr() + 8 * FRONT, cap_groups, *refs))
    host = [t.cpu().numpy() for t in (out, oo, di, ki, go)]
    for t, g in zip(host, (GUARD8, GUARD64, GUARD64, GUARD8, GUARD64)):
        assert (t[:FRONT] == g).all(), "a store in front of an output"
    assert (host[0][:lead] == GUARD8).all(), "a store in front of the output bytes"
    return (tuple(int(x.value) for x in cnt), host[0][lead:]) + tuple(t[FRONT:] for t in host[1:])


def check_raw(eng, d, out_at):
    c = d.c
    data, off, idx, kd, go = X.expected()[c.name]
    (m, hits, groups, total), out, oo, di, ki, gg = raw_context(eng, d, out_at=out_at)
    assert (m, hits, groups, total) == (len(idx), sum(kd), len(go) - 1, len(data)), c.name
    assert out[:total].tobytes() == data and (out[total:] == GUARD8).all(), (c.name, out_at)
    assert oo[:m + 1].tolist() == off and (oo[m + 1:] == GUARD64).all() and di[:m].tolist() == idx and (di[m:] == GUARD64).all(), (c.name, out_at)
    assert ki[:m].tolist() == kd and (ki[m:] == GUARD8).all() and gg[:groups + 1].tolist() == go and (gg[groups + 1:] == GUARD64).all(), (c.name, out_at)


def test_the_cases_are_not_vacuous():
    assert X.assert_not_vacuous()


def test_fixed_cases(eng):
    want, walk = X.expected(), host_walk()
    for i, c in enumerate(X.fixed_cases()):
        assert walk[c.name] == want[c.name], c.name
        for at, out_at in RESIDUES:
            d = OnDevice(c, at, 0xFF if i % 2 else 0)
            assert on_host(d.call(eng)) == want[c.name], (c.name, at)
            check_raw(eng, d, out_at)


def test_random_batches(eng):
    want, walk = X.expected(), host_walk()
    for i, c in enumerate(X.random_cases()):
        assert walk[c.name] == want[c.name], c.name
        at, out_at = RESIDUES[i % 3]
        d = OnDevice(c, at, 0xFF if i % 2 else 0)
        assert on_host(d.call(eng)) == want[c.name], c.name
        check_raw(eng, d, out_at)


def test_cap_protocol(eng):
    c = next(c for c in X.fixed_cases() if c.name == "65 documents, fences")
    data, off, idx, kd, go = X.expected()[c.name]
    total, m, g = len(data), len(idx), len(go) - 1
    assert m >= 4 and g >= 3
    k3 = next(k for k in range(m) if off[k + 1] - off[k] >= 2)
    mid = off[k3] + 1                                               # inside a document
    d = OnDevice(c, 3)
    for out_at, cb, cd, cg in [(0, total, m, g), (5, total - 1, m, g), (0, mid, m, g), (5, 1, m, g), (0, 0, m, g),
                               (0, total, m - 1, g), (5, total, 1, g), (0, total, 0, g),
                               (5, total, m, g - 1), (0, total, m, 1), (5, total, m, 0), (3, mid, 1, 1), (0, 0, 0, 0)]:
        cnt, out, oo, di, ki, gg = raw_context(eng, d, cb, cd, cg, out_at)
        assert cnt == (m, sum(kd), g, total), (cb, cd, cg)
        assert out[:cb].tobytes() == data[:cb] and (out[cb:] == GUARD8).all(), (cb, cd, cg)
        k, j = min(m, cd), min(g, cg)
        assert oo[:k + 1].tolist() == off[:k + 1] and (oo[k + 1:] == GUARD64).all(), (cb, cd, cg)
        assert di[:k].tolist() == idx[:k] and (di[k:] == GUARD64).all() and ki[:k].tolist() == kd[:k] and (ki[k:] == GUARD8).all(), (cb, cd, cg)
        assert gg[:j + 1].tolist() == go[:j + 1] and (gg[j + 1:] == GUARD64).all(), (cb, cd, cg)
    # a cap past the total: nothing behind the total is touched
    cnt, out, _, _, _, _ = raw_context(eng, d, total + 40, m, g, 7)
    assert out[:total].tobytes() == data and (out[total:] == GUARD8).all()


def test_count_only_and_no_documents(eng):
    L = _lib.load()
    c = next(c for c in X.fixed_cases() if c.name == "a fence inside a run of context")
    data, off, idx, kd, go = X.expected()[c.name]
    d = OnDevice(c)
    W = (c.n_cols + 31) // 32
    cnt = [C.c_uint64(9) for _ in range(4)]
    refs = [C.byref(x) for x in cnt]
    torch.cuda.synchronize()
    assert L.gft_context_docs_device(eng._h, d.text.data_ptr(), d.off.data_ptr(), d.n, d.rows.data_ptr(), c.n_cols, _want_words(c.want, c.n_cols).ctypes.data,
                                     0, None, c.before, c.after, d.fence.data_ptr(), None, 0, None, None, None, 0, None, 0, *refs) == 0
    assert [x.value for x in cnt] == [len(idx), sum(kd), len(go) - 1, len(data)] and W == 2
    # the counters are optional
    assert L.gft_context_docs_device(eng._h, d.text.data_ptr(), d.off.data_ptr(), d.n, d.rows.data_ptr(), c.n_cols, None, 0, None, 1, 1, None, None, 0, None,
                                     None, None, 0, None, 0, None, None, None, None) == 0
    # no documents: both offset arrays get their leading 0 and nothing else
    oo = torch.full((4,), GUARD64, dtype=torch.int64, device="cuda")
    go_t = torch.full((4,), GUARD64, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert L.gft_context_docs_device(eng._h, None, None, 0, None, 5, None, 0, None, 3, 3, None, None, 0, oo.data_ptr(), None, None, 0, go_t.data_ptr(), 0,
                                     *refs) == 0
    assert [x.value for x in cnt] == [0, 0, 0, 0] and oo.cpu().tolist() == [0] + [GUARD64] * 3 and go_t.cpu().tolist() == [0] + [GUARD64] * 3
    # nothing selected: nothing written, group_off[0] = 0
    c = next(c for c in X.fixed_cases() if c.name == "nothing selected")
    cnt, out, oo, di, ki, gg = raw_context(eng, OnDevice(c), 10, 4, 4)
    assert cnt == (0, 0, 0, 0) and (out == GUARD8).all() and oo.tolist() == [0] + [GUARD64] * 36 and (di == GUARD64).all() and (ki == GUARD8).all()
    assert gg.tolist() == [0] + [GUARD64] * 36


def test_refusals_leave_the_handle_usable(eng):
    L = _lib.load()
    E = _lib.GFT_E_INVALID
    c = next(c for c in X.fixed_cases() if c.name == "33 columns, any, also" or c.name == "70 columns, any, also")
    d = OnDevice(c)
    data, off, idx, kd, go = X.expected()[c.name]
    W = (c.n_cols + 31) // 32
    out = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda")
    oo = torch.zeros(len(idx) + 1, dtype=torch.int64, device="cuda")
    di = torch.zeros(len(idx), dtype=torch.int64, device="cuda")
    ki = torch.zeros(len(idx), dtype=torch.uint8, device="cuda")
    gg = torch.zeros(len(go), dtype=torch.int64, device="cuda")
    cnt = [C.c_uint64(0) for _ in range(4)]
    torch.cuda.synchronize()

    def call(text=d.text.data_ptr(), doc_off=d.off.data_ptr(), rows=d.rows.data_ptr(), mode=0, o=out.data_ptr(), cb=len(data), oop=oo.data_ptr(),
             dip=di.data_ptr(), kip=ki.data_ptr(), cd=len(idx), gop=gg.data_ptr(), cg=len(go) - 1):
        return L.gft_context_docs_device(eng._h, text, doc_off, d.n, rows, c.n_cols, c.want.ctypes.data, mode, d.also.data_ptr(), c.before, c.after,
                                         d.fence.data_ptr(), o, cb, oop, dip, kip, cd, gop, cg, *[C.byref(x) for x in cnt])
    assert call() == 0 and [x.value for x in cnt] == [len(idx), sum(kd), len(go) - 1, len(data)]
    assert call(text=None) == E and call(doc_off=None) == E and call(rows=None) == E         # a null argument
    assert "null argument" in L.gft_last_error(eng._h).decode()
    assert call(mode=3) == E                                                                 # unknown mode
    assert "gft_context_docs_device: unknown mode" in L.gft_last_error(eng._h).decode()
    assert L.gft_last_error(eng._h).decode() == "gft_context_docs_device: unknown mode"
    assert call(cd=1 << 61) == E                                                 # a size beyond the address space
    assert L.gft_last_error(eng._h).decode() == "gft_context_docs_device: a size beyond the address space"
    assert call(o=None) == E and call(oop=None) == E and call(dip=None) == E and call(kip=None) == E and call(gop=None) == E      # a cap without its array
    assert call(o=d.text.data_ptr() + int(c.doc_off[0]), cb=3) == E                          # the output over the text ...
    assert call(o=d.off.data_ptr(), cb=3) == E                                               # ... the offsets ...
    assert call(o=d.rows.data_ptr() + 4 * W * (d.n - 1), cb=3) == E                          # ... the last row ...
    assert call(o=d.also.data_ptr() + d.n - 1, cb=1) == E                                    # ... the last byte of `also` ...
    assert call(o=d.fence.data_ptr() + d.n - 1, cb=1) == E                                   # ... and of the fences
    assert call(oop=d.rows.data_ptr()) == E and call(dip=d.off.data_ptr()) == E and call(kip=d.fence.data_ptr()) == E
    assert call(gop=d.off.data_ptr()) == E and call(gop=oo.data_ptr()) == E and call(kip=out.data_ptr()) == E       # two outputs
    assert "overlaps" in L.gft_last_error(eng._h).decode()
    assert L.gft_last_error(eng._h).decode() == "gft_context_docs_device: an output overlaps an input"
    down = d.off.clone()
    down[3], down[4] = d.off[4].item(), d.off[3].item()
    if down[3] == down[4]:
        down[4] -= 1
    torch.cuda.synchronize()
    assert call(doc_off=down.data_ptr()) == E                                                # offsets that descend
    assert "gft_context_docs_device: document offsets descend" in L.gft_last_error(eng._h).decode()
    assert L.gft_last_error(eng._h).decode() == "gft_context_docs_device: document offsets descend, or a document of 4 GiB or more"
    huge = d.off.clone()
    huge[d.n] += 1 << 32
    torch.cuda.synchronize()
    assert call(doc_off=huge.data_ptr(), o=None, cb=0, oop=None, dip=None, kip=None, cd=0, gop=None, cg=0) == E      # a document of 4 GiB or more
    assert L.gft_last_error(eng._h).decode() == "gft_context_docs_device: document offsets descend, or a document of 4 GiB or more"
    with pytest.raises(ValueError):
        eng.context_docs_device(d.text, d.off, d.rows, c.n_cols, np.zeros(W + 1, np.uint32))
    with pytest.raises(ValueError):
        eng.context_docs_device(d.text, d.off, d.rows, c.n_cols, c.want, fence=d.fence[:-1].contiguous())
    with pytest.raises(ValueError):
        eng.context_docs_device(d.text, d.off, d.rows, c.n_cols, c.want, before=-1)
    assert on_host(d.call(eng)) == (data, off, idx, kd, go)


def test_profile_names_and_the_verdict_is_left_alone(eng):
    L = _lib.load()
    before = L.gft_last_nonascii(eng._h)
    d = OnDevice(next(c for c in X.random_cases() if len(X.expected()[c.name][0]) > 0))
    eng.profile(True)
    eng.profile_reset()
    d.call(eng)
    names = ("context_mark", "context_reach", "context_carry", "context_decide", "context_scan", "context_place", "context_copy")
    counts = {name: eng.profile_read(name)[1] for name in names}
    eng.profile(False)
    assert counts == dict({name: 2 for name in names}, context_copy=1)                       # (count only, then the fill)
    assert L.gft_last_nonascii(eng._h) == before


def test_handles_over_several_devices_are_refused():
    c = X.fixed_cases()[0]
    d = OnDevice(c)
    e = Engine(devices=[0, 0])
    with pytest.raises(GftError) as ei:
        d.call(e)
    assert ei.value.code == _lib.GFT_E_UNSUPPORTED
    e.close()
    one = Engine()
    assert on_host(d.call(one)) == X.expected()[c.name]
    one.close()


def test_without_reach_and_fence_it_is_the_select(eng):
    for c in S.fixed_cases() + S.random_cases()[6:]:
        d = OnDevice(c)
        out, out_off, doc_idx = eng.select_docs_device(d.text, d.off, d.rows, c.n_cols, c.want, c.mode, d.also)
        kout, koff, kidx, kind, group_off = d.call(eng)
        assert torch.equal(kout, out) and torch.equal(koff, out_off) and torch.equal(kidx, doc_idx), c.name
        assert bool((kind == 1).all()), c.name
        idx = doc_idx.cpu().tolist()
        runs = [r for r in range(len(idx)) if r == 0 or idx[r - 1] != idx[r] - 1]
        assert group_off.cpu().tolist() == runs + [len(idx)], c.name


def test_a_text_past_four_gib(eng):
    """one case whose documents begin past position 2^32 of their allocation; at the same positions modulo 2^32 lies poison, which a
    source address cut to 32 bits would copy"""
    c = next(c for c in X.fixed_cases() if c.name == "text that begins at 7")
    size = int(c.doc_off[-1])
    need = F.B + size + F.SLACK + 32
    free, _ = torch.cuda.mem_get_info()
    if free < need + (1 << 30):
        pytest.skip("the device has %d MiB free, the text past 4 GiB needs %d MiB" % (free >> 20, (need + (1 << 30)) >> 20))
    buf = torch.empty(need, dtype=torch.uint8, device="cuda")
    at = F.B + 9
    buf[:size + 128] = F.POISON
    buf[at:at + size + F.SLACK] = F.POISON
    lead = int(c.doc_off[0])
    buf[at + lead:at + size] = torch.from_numpy(c.blob[lead:size].copy()).cuda()
    off = torch.from_numpy((c.doc_off + np.uint64(at)).astype(np.int64)).cuda()
    rows = torch.from_numpy(c.rows.view(np.int32).copy()).cuda()
    fence = torch.from_numpy(c.fence).cuda()
    assert int(off[0]) > 1 << 32
    got = on_host(eng.context_docs_device(buf, off, rows, c.n_cols, c.want, c.mode, None, c.before, c.after, fence))
    assert got == X.expected()[c.name]
    del buf
    torch.cuda.empty_cache()


# ---- the finder -----------------------------------------------------------------------------------------------------------------
def lines_finder(n=2000, whole_words=False):
    w = Workload(n)
    text, off = w.docs_host(0, n)
    docs = [bytes(text[int(off[i]):int(off[i + 1])]).replace(b"\n", b" ") for i in range(n)]
    terms = [t.decode("ascii") for t in w.terms() if t.isalpha()][:40]
    docs[7] = b""                                                      # an empty line
    f = Finder(GpuEngine(), EmptyRgxEngine(), False, whole_words=whole_words)
    for i, t in enumerate(terms[:6]):
        f.AddExpressionWithTag('"%s"' % t, "tag%d" % (i % 3))
    f.AddExpressionWithTag('"école" and "%s"' % terms[1], "french")
    f.AddExpressionWithTag('"%s" and not "%s"' % (terms[2], terms[3]), "tag0")
    return f, docs, terms


def check_lines(f, blob, masks, lowered_repeats):
    pieces = SL.documents(blob, SL.AFTER_NL)
    rows = f.ProcessTexts(pieces)
    off = SL.reference(blob, SL.AFTER_NL)
    E = f.n_expressions
    seen = f.lowered_batches()
    telling = 0
    for want, mode, before, after in masks:
        ref = X.reference(blob, off, rows, E, want, mode, None, before, after, None)
        telling += 0 < len(ref[2]) < len(pieces) and 0 in ref[3] and 1 in ref[3] and len(ref[4]) > 2
        r = f.ContextLinesDevice(resident(blob, 3), len(blob), before, after, want, mode)
        assert on_host(r[:5]) == ref, (mode, before, after)
        assert r[5].cpu().tolist() == off and np.array_equal(r[6].cpu().numpy().view(np.uint32), rows)
        h = f.ContextLines(blob, before, after, want, mode)
        assert (h[0], h[1].tolist(), h[2].tolist(), h[3].tolist(), h[4].tolist()) == ref, (mode, before, after)
    now = f.lowered_batches()
    assert now[0] - seen[0] == (2 * len(masks) if lowered_repeats else 0), "the lowering repeat"
    assert telling, "no mask keeps some lines as hits, some as context, in several groups"
    return rows


def test_finder_context_lines_on_an_ascii_log():
    f, docs, terms = lines_finder()
    blob = b"\n".join(docs) + b"\n"
    check_lines(f, blob, [(None, "any", 2, 2), (f.want_mask(indices=[0, 5]), "any", 0, 3), (f.want_mask(tags=["tag1"]), "any", 1, 0),
                          (f.want_mask(indices=[2, 3]), "all", 1, 1), (f.want_mask(indices=[0]), "any", 0, 0)], False)
    out = f.ContextLines(b"", 2, 2)
    assert out[0] == b"" and out[1].tolist() == [0] and out[2].size == 0 and out[3].size == 0 and out[4].tolist() == [0]
    f.close()


def test_finder_context_lines_on_a_log_that_leaves_ascii():
    f, docs, terms = lines_finder()
    docs[20] = ("VIVE LA École " + terms[1].upper()).encode("utf-8")   # upper-case non-ASCII: lowered on the device, scanned again
    blob = b"\n".join(docs) + b"\n"
    french = f.want_mask(tags=["french"])
    rows = check_lines(f, blob, [(french, "any", 1, 2), (None, "any", 1, 1)], True)
    assert X.reference(blob, SL.reference(blob, SL.AFTER_NL), rows, f.n_expressions, french, "any", None, 1, 2, None)[2] == [19, 20, 21, 22]
    f.close()


def test_finder_context_lines_with_whole_words():
    f, docs, terms = lines_finder(whole_words=True)
    g, _, _ = lines_finder(whole_words=False)
    blob = b"\n".join(docs) + b"\n"
    rows = check_lines(f, blob, [(None, "any", 1, 1), (f.want_mask(indices=[0, 1]), "any", 0, 2)], False)
    loose = g.ProcessTexts(SL.documents(blob, SL.AFTER_NL))
    assert not ((rows & 0x3F) & ~(loose & 0x3F)).any()                                       # the single-keyword columns: word borders only drop hits
    f.close()
    g.close()
    # `he` in "ushers" and "the" is no word: line 1 alone hits, line 2 is its context
    for whole, kept, kind in ((True, [1, 2], [1, 0]), (False, [0, 1, 2, 3], [1, 1, 1, 0])):
        h = Finder(GpuEngine(), EmptyRgxEngine(), False, whole_words=whole)
        h.AddExpression('"he"')
        got = h.ContextLines(b"ushers\nhe\nthe\nx\ny\n", 0, 1)
        assert got[2].tolist() == kept and got[3].tolist() == kind and got[4].tolist() == [0, len(kept)], whole
        dev = h.ContextLinesDevice(resident(b"ushers\nhe\nthe\nx\ny\n"), 18, 0, 1)
        assert dev[2].cpu().tolist() == kept and dev[3].cpu().tolist() == kind
        h.close()


def test_finder_context_lines_inverted():
    """mode "none": grep -v with context"""
    f, docs, terms = lines_finder()
    # most lines carry the first keyword: the lines that do not are the hits of the inverted search
    docs = [d if i % 7 == 3 else d + b" " + terms[0].encode() for i, d in enumerate(docs[:400])]
    blob = b"\n".join(docs) + b"\n"
    check_lines(f, blob, [(f.want_mask(indices=[0]), "none", 1, 1), (f.want_mask(indices=[0, 6]), "none", 0, 1)], False)
    f.close()


def test_finder_context_needs_what_process_device_needs():
    from gofindthem_amd.finder import PyRegexpEngine
    f = Finder(GpuEngine(), PyRegexpEngine(), False)
    f.AddExpressions(['"ab"', 'r"c+d"'])
    buf = resident(b"ab\ncd\nxx\n")
    off = torch.tensor([0, 3, 6, 9], dtype=torch.int64, device="cuda")
    rows = torch.zeros((3, 1), dtype=torch.int32, device="cuda")
    with pytest.raises(FinderError) as e1:
        f.ContextDevice(buf, off, rows, before=1)
    with pytest.raises(FinderError) as e2:
        f.SelectDevice(buf, off, rows)
    assert e1.value.code == e2.value.code == _lib.GFT_E_UNSUPPORTED and str(e1.value) == str(e2.value)
    got = f.ContextLines(b"ab\ncd\nxx\nyy\nccd ab\n", 0, 1)                                # the host-memory form goes on answering
    assert got[0] == b"ab\ncd\nxx\nccd ab\n" and got[2].tolist() == [0, 1, 2, 4] and got[3].tolist() == [1, 1, 0, 1] and got[4].tolist() == [0, 3, 4]
    f.close()


def test_context_between_begin_and_end_only_after_complete():
    f, docs, terms = lines_finder()
    blob = b"\n".join(docs) + b"\n"
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
    ref = X.reference(blob, off.cpu().tolist(), rows.cpu().numpy().view(np.uint32), f.n_expressions, want, "any", None, 1, 1, None)
    assert 0 < len(ref[2]) < n
    cnt = [C.c_uint64(0) for _ in range(4)]
    args = (buf.data_ptr(), off.data_ptr(), n, rows.data_ptr(), f.n_expressions, want.ctypes.data, 0, None, 1, 1, None, None, 0, None, None, None, 0, None, 0,
            *[C.byref(x) for x in cnt])
    torch.cuda.synchronize()
    f.ProcessDeviceBegin(buf.data_ptr(), off.data_ptr(), n, bm.data_ptr())
    assert L.gft_context_docs_device(eh, *args) == _lib.GFT_E_INVALID
    assert "in flight" in L.gft_last_error(eh).decode()
    with pytest.raises(FinderError):
        f.ContextDevice(buf, off, rows, want, before=1, after=1)         # the finder's form waits for ProcessDeviceEnd
    assert L.gft_process_device_complete(eh) == 0
    assert L.gft_context_docs_device(eh, *args) == 0 and [x.value for x in cnt] == [len(ref[2]), sum(ref[3]), len(ref[4]) - 1, len(ref[0])]
    f.ProcessDeviceEnd()
    assert torch.equal(bm, rows)
    assert on_host(f.ContextDevice(buf, off, rows, want, before=1, after=1)) == ref
    f.close()
