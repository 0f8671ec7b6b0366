"""Documents routed to per-bucket runs of one blob on the device (csrc/gft_route.hip): Engine.route_docs_device and the raw C call
against the reference of route_docs.py AND the host walk, byte for byte and entry for entry, on every fixed case (the borders come
from route_shape()) and on seeded random batches, with the text and the output at four residues of the 16-byte grid; the cap
protocol into guarded tensors; the refusals; every bucket against select_docs_device; and the callers -- Finder.RouteLines /
CountLines against per-line ProcessText, GroupFinder.RouteJsonLines against ProcessJsons over the lines."""
import ctypes as C
import functools
import json

import numpy as np
import pytest
import torch  # noqa: F401  (before libgft.so is loaded: one HIP runtime)

import route_docs as R
from gofindthem_amd import _lib, group
from gofindthem_amd.engine import Engine, GftError, route_docs_host, route_shape, _mask_rows
from gofindthem_amd.finder import EmptyRgxEngine, Finder, FinderError, GpuEngine, PyRegexpEngine

pytestmark = pytest.mark.gpu

GUARD8, GUARD64 = 0xFF, -0x5A5A5A5A5A5A5A5B
RESIDUES = (0, 1, 8, 15)


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
    """a case of route_docs.py on the device, its text `at` bytes into its allocation"""

    def __init__(self, c, at=0, fill=0):
        self.c = c
        self.text = resident(c.blob.tobytes(), at, fill)
        self.off = torch.from_numpy(c.doc_off.astype(np.int64)).cuda()
        self.rows = torch.from_numpy(c.rows.view(np.int32).copy()).cuda()
        self.also = torch.from_numpy(c.also).cuda() if c.also is not None else None
        self.n = len(c.doc_off) - 1


@functools.lru_cache(maxsize=None)
def host_walk():
    """{name: (bytes, out_off, doc_idx, bucket_doc, bucket_byte)} of gft_debug_route_docs, computed once"""
    out = {}
    for c in R.all_cases():
        bd, bb, data, off, idx = route_docs_host(c.blob, c.doc_off, c.rows, c.n_cols, c.masks, c.mode, c.rest, c.also)
        m, total = int(bd[-1]), int(bb[-1])
        out[c.name] = (data[:total].tobytes(), off[:m + 1].tolist(), idx[:m].tolist(), bd.tolist(), bb.tolist())
    return out


def raw_route(eng, d, cap_bytes=None, cap_docs=None, out_at=0, guard=32, mode=None, flags=None, masks=None, also="own"):
    """gft_route_docs_device into guarded tensors, the output `out_at` bytes into its allocation -> (bucket_doc, bucket_byte, out,
    out_off, doc_idx) on the host, guards included.  Caps None: count first"""
    L = _lib.load()
    c = d.c
    W = (c.n_cols + 31) // 32
    K, w = _mask_rows(c.masks if masks is None else masks, c.n_cols)
    B = K + (1 if c.rest else 0)
    also = d.also if isinstance(also, str) else also
    head = (eng._h, d.text.data_ptr(), d.off.data_ptr(), d.n, d.rows.data_ptr() if W and d.n else None, c.n_cols, w.ctypes.data, K,
            R.MODES[c.mode] if mode is None else mode, (1 if c.rest else 0) if flags is None else flags, also.data_ptr() if also is not None else None)
    bd, bb = np.full(B + 1, 99, np.uint64), np.full(B + 1, 99, np.uint64)
    torch.cuda.synchronize()
    if cap_bytes is None:
        eng._check(L.gft_route_docs_device(*head, None, 0, None, None, 0, bd.ctypes.data, bb.ctypes.data))
        cap_bytes, cap_docs = int(bb[B]), int(bd[B])
    out = torch.full((out_at + cap_bytes + guard,), GUARD8, dtype=torch.uint8, device="cuda")
    oo = torch.full((cap_docs + 1 + guard,), GUARD64, dtype=torch.int64, device="cuda")
    di = torch.full((cap_docs + guard,), GUARD64, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    eng._check(L.gft_route_docs_device(*head, out.data_ptr() + out_at, cap_bytes, oo.data_ptr(), di.data_ptr(), cap_docs, bd.ctypes.data, bb.ctypes.data))
    return bd.tolist(), bb.tolist(), out.cpu().numpy(), oo.cpu().numpy(), di.cpu().numpy()


def check_raw(eng, d, out_at):
    c = d.c
    data, off, idx, bd, bb = R.expected()[c.name]
    m, total = len(idx), len(data)
    gd, gb, out, oo, di = raw_route(eng, d, out_at=out_at)
    assert (gd, gb) == (bd, bb), c.name
    assert (out[:out_at] == GUARD8).all() and out[out_at:out_at + total].tobytes() == data and (out[out_at + total:] == GUARD8).all(), (c.name, out_at)
    assert oo[:m + 1].tolist() == off and (oo[m + 1:] == GUARD64).all() and di[:m].tolist() == idx and (di[m:] == GUARD64).all(), (c.name, out_at)


def check_engine(eng, d):
    c = d.c
    data, off, idx, bd, bb = R.expected()[c.name]
    assert host_walk()[c.name] == (data, off, idx, bd, bb), c.name
    out, out_off, doc_idx, bucket_doc, bucket_byte = eng.route_docs_device(d.text, d.off, d.rows, c.n_cols, c.masks, c.mode, c.rest, d.also)
    assert out.cpu().numpy().tobytes() == data and out_off.cpu().tolist() == off and doc_idx.cpu().tolist() == idx, c.name
    assert bucket_doc.tolist() == bd and bucket_byte.tolist() == bb, c.name


def test_the_cases_are_not_vacuous():
    assert R.assert_not_vacuous()
    T = route_shape()
    sizes = set(len(c.doc_off) - 1 for c in R.fixed_cases())
    assert {1, T - 1, T, T + 1, 2 * T + 1, 65 * T} <= sizes
    want = R.expected()
    bd = want["buckets 0, 2 and 4 stay empty"][3]
    assert bd[0] == bd[1] < bd[2] == bd[3] < bd[4] == bd[5]
    assert want["every document in the last bucket"][3][63:] == [0, T + 5]
    all64 = want["a document in all 64 buckets"][2]
    assert all64.count(T - 1) == 64
    assert 1 in want["a document hits buckets 3 and 7, every"][2][want["a document hits buckets 3 and 7, every"][3][7]:]
    first = want["a document hits buckets 3 and 7, first"]
    assert first[2][first[3][3]:first[3][4]] == [1, 2] and first[2][first[3][7]:first[3][8]] == [0]
    assert want["no rest and no hit"][2] == [] and want["no rest, one document absent"][2] == [0, 2]
    assert want["no masks, no rest"][3] == [0] and want["no masks, rest"][3] == [0, 3]
    assert want["only the last document is routed"][2] == [2 * T]
    for mode in ("first", "every"):
        a = want["also, %s" % mode]
        rest = a[2][a[3][6]:]
        assert {0, 5, 6, 40, 79} <= set(rest) and not {0, 5, 40} & set(a[2][:a[3][6]])
    assert len(want["64 buckets, 65 tiles"][2]) > 4096 and len(want["5000 entries in two buckets"][2]) > 4096
    for n_cols in (31, 32, 33, 40, 65, 2048, 2080):                  # hits in the last valid bit and in the last word's first bit
        bd = want["%d columns, every" % n_cols][3]
        assert bd[1] > 0 and bd[2] > bd[1]
    assert want["0 columns, every"][3] == [0, 0, 0, 0, 150]


def test_fixed_cases(eng):
    for c in R.fixed_cases():
        check_engine(eng, OnDevice(c))


def test_no_documents(eng):
    L = _lib.load()
    for flags in (0, 1):
        bd, bb = np.full(5, 9, np.uint64), np.full(5, 9, np.uint64)
        oo = torch.full((4,), GUARD64, dtype=torch.int64, device="cuda")
        masks = np.ones(3, np.uint32)
        torch.cuda.synchronize()
        assert L.gft_route_docs_device(eng._h, None, None, 0, None, 5, masks.ctypes.data, 3, 1, flags, None, None, 0, oo.data_ptr(), None, 0, bd.ctypes.data,
                                       bb.ctypes.data) == 0
        assert bd[:4 + flags].tolist() == [0] * (4 + flags) and bb[:4 + flags].tolist() == [0] * (4 + flags) and oo.cpu().tolist() == [0] + [GUARD64] * 3


@pytest.mark.parametrize("fill", [0, 0xFF], ids=["zeros behind", "ones behind"])
def test_text_and_output_at_four_residues_and_what_the_slack_holds(eng, fill):
    names = ["%d documents" % (2 * route_shape() + 1), "empty documents at a bucket's borders and as a whole bucket", "63 masks, rest", "65 columns, every",
             "2080 columns, first", "also, every", "doc_off[0] = 5"]
    for name in names:
        c = R.case(name)
        for i, at in enumerate(RESIDUES):
            d = OnDevice(c, at, fill)
            check_engine(eng, d)
            check_raw(eng, d, RESIDUES[(i + 2) % 4])
        d = OnDevice(c, 0, fill)
        for out_at in RESIDUES:
            check_raw(eng, d, out_at)


def test_random_batches(eng):
    for i, c in enumerate(R.random_cases()[:60]):
        d = OnDevice(c, RESIDUES[i % 4], 0xFF)
        check_engine(eng, d)
        check_raw(eng, d, RESIDUES[(i + 1) % 4])


def test_cap_protocol(eng):
    c = R.case("%d documents" % (2 * route_shape() + 1))
    data, off, idx, bd, bb = R.expected()[c.name]
    total, m = len(data), len(idx)
    in_bucket_1 = (bb[1] + bb[2]) // 2
    in_bucket_0 = bd[1] // 2
    assert bb[1] < in_bucket_1 < bb[2] and 0 < in_bucket_0 < bd[1]
    d = OnDevice(c, 3)
    for out_at in (0, 5):
        for cb in (total, total - 1, in_bucket_1, 1, 0):
            for cd in (m, in_bucket_0, 0):
                gd, gb, out, oo, di = raw_route(eng, d, cb, cd, out_at)
                assert (gd, gb) == (bd, bb), (cb, cd)
                k = min(m, cd)
                assert (out[:out_at] == GUARD8).all() and out[out_at:out_at + cb].tobytes() == data[:cb] and (out[out_at + cb:] == GUARD8).all(), (cb, cd)
                assert oo[:k + 1].tolist() == off[:k + 1] and (oo[k + 1:] == GUARD64).all(), (cb, cd)
                assert di[:k].tolist() == idx[:k] and (di[k:] == GUARD64).all(), (cb, cd)
    # a cap past the total: nothing behind the total is touched
    _, _, out, _, _ = raw_route(eng, d, total + 40, m, 7)
    assert out[7:7 + total].tobytes() == data and (out[7 + total:] == GUARD8).all()
    # count only: the host arrays alone; and nothing at all
    got = eng.route_count_device(d.text, d.off, d.rows, c.n_cols, c.masks, c.mode, c.rest, d.also)
    assert got[0].tolist() == bd and got[1].tolist() == bb
    K, w = _mask_rows(c.masks, c.n_cols)
    torch.cuda.synchronize()
    assert _lib.load().gft_route_docs_device(eng._h, d.text.data_ptr(), d.off.data_ptr(), d.n, d.rows.data_ptr(), c.n_cols, w.ctypes.data, K, 1, 1, None,
                                             None, 0, None, None, 0, None, None) == 0


def test_refusals_leave_the_handle_usable(eng):
    L = _lib.load()
    E, U = _lib.GFT_E_INVALID, _lib.GFT_E_UNSUPPORTED
    c = R.case("also, every")
    d = OnDevice(c)
    data, off, idx, bd, bb = R.expected()[c.name]
    W = (c.n_cols + 31) // 32
    K, w = _mask_rows(c.masks, c.n_cols)
    out = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda")
    oo = torch.zeros(len(idx) + 1, dtype=torch.int64, device="cuda")
    di = torch.zeros(len(idx), dtype=torch.int64, device="cuda")
    hd, hb = np.zeros(67, np.uint64), np.zeros(67, np.uint64)
    many = np.ascontiguousarray(np.tile(w[:W], 65))
    torch.cuda.synchronize()

    def call(text=d.text.data_ptr(), doc_off=d.off.data_ptr(), masks=w.ctypes.data, k=K, mode=1, flags=1, also=d.also.data_ptr(), o=out.data_ptr(),
             cb=len(data), oop=oo.data_ptr(), dip=di.data_ptr(), cd=len(idx)):
        return L.gft_route_docs_device(eng._h, text, doc_off, d.n, d.rows.data_ptr(), c.n_cols, masks, k, mode, flags, also, o, cb, oop, dip, cd,
                                       hd.ctypes.data, hb.ctypes.data)
    assert call() == 0 and hd[:K + 2].tolist() == bd
    assert call(mode=2) == E                                                     # unknown mode
    assert L.gft_last_error(eng._h).decode() == "gft_route_docs_device: unknown mode"
    assert call(cd=1 << 61) == E                                                 # a size beyond the address space
    assert L.gft_last_error(eng._h).decode() == "gft_route_docs_device: a size beyond the address space"
    assert call(flags=2, also=None) == E and call(flags=3) == E                  # unknown flag bits
    assert call(flags=0) == E                                                    # also without rest
    assert "GFT_ROUTE_REST" in L.gft_last_error(eng._h).decode()
    assert L.gft_last_error(eng._h).decode() == "gft_route_docs_device: d_also needs GFT_ROUTE_REST"
    assert call(flags=0, also=None) == 0
    assert call(masks=many.ctypes.data, k=65, flags=0, also=None) == U           # 65 buckets
    assert "64" in L.gft_last_error(eng._h).decode()
    assert call(masks=many.ctypes.data, k=64) == U                               # 64 and the rest
    assert call(masks=many.ctypes.data, k=64, flags=0, also=None, o=None, cb=0, oop=None, dip=None, cd=0) == 0
    assert call(masks=None) == E
    assert call(o=None) == E and call(oop=None) == E and call(dip=None) == E     # a cap without its array
    assert call(o=d.text.data_ptr() + int(c.doc_off[0]), cb=3) == E              # the output over the text ...
    assert call(o=d.off.data_ptr(), cb=3) == E                                   # ... the offsets ...
    assert call(o=d.rows.data_ptr() + 4 * W * (d.n - 1), cb=3) == E              # ... the last row ...
    assert call(o=d.also.data_ptr() + d.n - 1, cb=1) == E                        # ... the last byte of `also`
    assert call(oop=d.rows.data_ptr()) == E and call(dip=d.off.data_ptr()) == E
    assert "overlaps" in L.gft_last_error(eng._h).decode()
    assert L.gft_last_error(eng._h).decode() == "gft_route_docs_device: an output overlaps an input"
    down = d.off.clone()
    down[3], down[4] = d.off[4].item(), d.off[3].item()
    if down[3] == down[4]:
        down[4] -= 1
    torch.cuda.synchronize()
    assert call(doc_off=down.data_ptr()) == E                                    # offsets that descend
    assert "descend" in L.gft_last_error(eng._h).decode()
    assert L.gft_last_error(eng._h).decode() == "gft_route_docs_device: document offsets descend, or a document of 4 GiB or more"
    huge = d.off.clone()
    huge[d.n] += 1 << 32
    torch.cuda.synchronize()
    assert call(doc_off=huge.data_ptr(), o=None, cb=0, oop=None, dip=None, cd=0) == E      # a document of 4 GiB or more
    assert L.gft_last_error(eng._h).decode() == "gft_route_docs_device: document offsets descend, or a document of 4 GiB or more"
    with pytest.raises(ValueError):
        eng.route_docs_device(d.text, d.off, d.rows, c.n_cols, np.zeros((2, W + 1), np.uint32))
    with pytest.raises(GftError) as ei:
        eng.route_docs_device(d.text, d.off, d.rows, c.n_cols, c.masks, c.mode, False, d.also)
    assert ei.value.code == E
    check_engine(eng, d)


def test_every_bucket_is_a_select(eng):
    """EVERY mode: bucket k's slice is what select_docs_device(want = masks[k], "any") returns, the rest bucket what "none" over the
    union of the masks returns -- bytes, offsets and indices -- on one random batch of a few thousand documents"""
    rng = np.random.default_rng(5)
    n, K, n_cols = 3000, 9, 70
    hits = [np.flatnonzero(rng.random(K) < 0.15).tolist() for _ in range(n)]
    lens = np.where(rng.random(n) < 0.8, rng.integers(0, 40, n), rng.integers(0, 3000, n)).tolist()
    c = R.make("select cross-check", lens, hits, K, rest=True, n_cols=n_cols, seed=77, lead=3)
    d = OnDevice(c, 5, 0xFF)
    out, out_off, doc_idx, bd, bb = eng.route_docs_device(d.text, d.off, d.rows, n_cols, c.masks, "every", True)
    out, out_off, doc_idx = out.cpu().numpy(), out_off.cpu().numpy(), doc_idx.cpu().numpy()
    union = np.bitwise_or.reduce(c.masks, axis=0)
    for k in range(K + 1):
        s_out, s_off, s_idx = eng.select_docs_device(d.text, d.off, d.rows, n_cols, union if k == K else c.masks[k], "none" if k == K else "any")
        a, b = int(bd[k]), int(bd[k + 1])
        assert b - a == s_idx.numel() > 0, k
        assert doc_idx[a:b].tolist() == s_idx.cpu().tolist(), k
        assert (out_off[a:b + 1] - out_off[a]).tolist() == s_off.cpu().tolist() and int(out_off[a]) == int(bb[k]), k
        assert out[int(bb[k]):int(bb[k + 1])].tobytes() == s_out.cpu().numpy().tobytes(), k
    assert int(bb[K + 1]) == out.size and int(bd[K + 1]) == doc_idx.size
    assert (out.tobytes(), out_off.tolist(), doc_idx.tolist(), bd.tolist(), bb.tolist()) == R.reference(c.blob, c.doc_off, c.rows, n_cols, c.masks, "every", True, None)


def test_profile_names_and_the_verdict_is_left_alone(eng):
    L = _lib.load()
    before = L.gft_last_nonascii(eng._h)
    c = R.case("64 buckets, 65 tiles")
    d = OnDevice(c)
    eng.profile(True)
    eng.profile_reset()
    eng.route_docs_device(d.text, d.off, d.rows, c.n_cols, c.masks, c.mode, c.rest, d.also)
    counts = {name: eng.profile_read(name)[1] for name in ("route_mark", "route_count", "route_scan", "route_place", "route_copy")}
    eng.profile(False)
    assert counts == {"route_mark": 2, "route_count": 2, "route_scan": 4, "route_place": 2, "route_copy": 1}     # (count only, then the fill)
    assert L.gft_last_nonascii(eng._h) == before


def test_handles_over_several_devices_are_refused():
    c = R.case("doc_off[0] = 5")
    d = OnDevice(c)
    e = Engine(devices=[0, 0])
    with pytest.raises(GftError) as ei:
        e.route_docs_device(d.text, d.off, d.rows, c.n_cols, c.masks, c.mode, c.rest)
    assert ei.value.code == _lib.GFT_E_UNSUPPORTED
    e.close()
    one = Engine()
    check_engine(one, d)
    one.close()


# ---- the finder -----------------------------------------------------------------------------------------------------------------
LOG = [b"2024-05-01 disk error on sda", b"all fine", b"warn: disk ok", b"", b"FATAL warn: giving up", b"network timeout, retry", b"error: network down",
       b"disk warn error network", b"disk almost full"] * 9 + [b"the last line has no newline: error"]
TAGGED = [('"error"', "err"), ('"warn"', "warn"), ('"disk" and not "ok"', "disk"), ('"fatal"', "err"), ('"network" or "timeout"', "net")]


def log_finder(regex=False):
    f = Finder(GpuEngine(), PyRegexpEngine() if regex else EmptyRgxEngine(), False)
    for e, t in TAGGED:
        f.AddExpressionWithTag(e, t)
    if regex:
        f.AddExpressionWithTag('r"no+ newline"', "net")
    return f


def by_process_text(f, lines, buckets, mode, rest):
    """the parts and indices from per-line ProcessText of the same finder: a bucket is a set of tags"""
    parts, idx = [[] for _ in range(len(buckets) + rest)], [[] for _ in range(len(buckets) + rest)]
    for i, line in enumerate(lines):
        tags = set(r.Tag for r in f.ProcessText(line.decode("utf-8")))
        hit = [k for k, b in enumerate(buckets) if tags & b]
        if mode == "first":
            hit = hit[:1]
        if rest and not hit:
            hit = [len(buckets)]
        for k in hit:
            parts[k].append(line)
            idx[k].append(i)
    return [b"".join(p) for p in parts], idx


def test_finder_route_lines_and_count_lines():
    f = log_finder()
    blob = b"\n".join(LOG)
    lines = [x + b"\n" for x in LOG[:-1]] + [LOG[-1]]
    assert f.tags() == ["err", "warn", "disk", "net"]
    for buckets, sets, mode, rest in ((None, [{"err"}, {"warn"}, {"disk"}, {"net"}], "every", False), (None, [{"err"}, {"warn"}, {"disk"}, {"net"}], "first", True),
                                      (["net", ["err", "disk"]], [{"net"}, {"err", "disk"}], "every", True)):
        want_parts, want_idx = by_process_text(f, lines, sets, mode, rest)
        parts, idx = f.RouteLines(blob, buckets, mode, rest)
        assert parts == want_parts and [i.tolist() for i in idx] == want_idx, (buckets, mode, rest)
        assert all(want_idx[:len(sets)]) and len(set(map(tuple, want_idx))) == len(want_idx)
    want_parts, want_idx = by_process_text(f, lines, [{"err"}, {"warn"}, {"disk"}, {"net"}], "every", False)
    docs, nbytes = f.CountLines(blob)
    assert docs.tolist() == [len(i) for i in want_idx] and nbytes.tolist() == [len(p) for p in want_parts]
    out, out_off, doc_idx, bd, bb, off, bm = f.RouteLinesDevice(resident(blob, 3), len(blob))
    assert doc_idx.cpu().tolist() == sum(want_idx, []) and out.cpu().numpy().tobytes() == b"".join(want_parts) and off.numel() == len(lines) + 1
    parts, idx = f.RouteLines(b"")
    assert parts == [b""] * 4 and [i.tolist() for i in idx] == [[]] * 4
    f.close()


def test_a_finder_with_a_regex_term_routes_on_the_host_walk():
    f, g = log_finder(), log_finder(regex=True)
    blob = b"\n".join(LOG)
    lines = [x + b"\n" for x in LOG[:-1]] + [LOG[-1]]
    assert g._takes_device_route() is False and f._takes_device_route() is True
    buf = resident(blob)
    off = torch.tensor([0, len(blob)], dtype=torch.int64, device="cuda")
    rows = torch.zeros((1, 1), dtype=torch.int32, device="cuda")
    with pytest.raises(FinderError) as e1:
        g.RouteDevice(buf, off, rows, g.route_masks())
    with pytest.raises(FinderError) as e2:
        g.SelectDevice(buf, off, rows)
    assert e1.value.code == e2.value.code == _lib.GFT_E_UNSUPPORTED and str(e1.value) == str(e2.value)
    # without the regex's own hits the two finders agree part for part: the buckets that do not hold the regex expression
    for mode, rest in (("every", False), ("first", True)):
        a, ai = f.RouteLines(blob, ["err", "warn", "disk"], mode, rest)
        b, bi = g.RouteLines(blob, ["err", "warn", "disk"], mode, rest)
        assert a == b and [i.tolist() for i in ai] == [i.tolist() for i in bi]
    sets = [{"err"}, {"warn"}, {"disk"}, {"net"}]
    want_parts, want_idx = by_process_text(g, lines, sets, "every", True)
    parts, idx = g.RouteLines(blob, None, "every", True)
    assert parts == want_parts and [i.tolist() for i in idx] == want_idx and len(lines) - 1 in want_idx[3]
    docs, nbytes = g.CountLines(blob)
    assert docs.tolist() == [len(i) for i in want_idx[:4]] and nbytes.tolist() == [len(p) for p in want_parts[:4]]
    f.close()
    g.close()


def test_route_between_begin_and_end_only_after_complete():
    f = log_finder()
    L = _lib.load()
    eh = f.engine_handle()
    blob = b"\n".join(LOG * 20) + b"\n"
    buf = resident(blob)
    off = f.SplitLinesDevice(buf, len(blob), 0)
    n = off.numel() - 1
    W = (f.n_expressions + 31) // 32
    bm = torch.zeros((n, W), dtype=torch.int32, device="cuda")
    for _ in range(4):                                                   # sizes learnt: the next batch runs deferred
        f.ProcessDevice(buf.data_ptr(), off.data_ptr(), n, bm.data_ptr())
    rows = bm.clone()
    masks = f.route_masks()
    want = R.reference(blob, off.cpu().tolist(), rows.cpu().numpy().view(np.uint32), f.n_expressions, masks, "every", False, None)
    K, w = _mask_rows(masks, f.n_expressions)
    bd, bb = np.zeros(K + 1, np.uint64), np.zeros(K + 1, np.uint64)
    args = (buf.data_ptr(), off.data_ptr(), n, rows.data_ptr(), f.n_expressions, w.ctypes.data, K, 1, 0, None, None, 0, None, None, 0, bd.ctypes.data,
            bb.ctypes.data)
    torch.cuda.synchronize()
    f.ProcessDeviceBegin(buf.data_ptr(), off.data_ptr(), n, bm.data_ptr())
    assert L.gft_route_docs_device(eh, *args) == _lib.GFT_E_INVALID
    assert "in flight" in L.gft_last_error(eh).decode()
    with pytest.raises(FinderError):
        f.RouteDevice(buf, off, rows, masks)                             # the finder's form waits for ProcessDeviceEnd
    assert L.gft_process_device_complete(eh) == 0
    assert L.gft_route_docs_device(eh, *args) == 0 and bd.tolist() == want[3] and bb.tolist() == want[4] and want[3][-1] > n // 2
    f.ProcessDeviceEnd()
    assert torch.equal(bm, rows)
    out, d_out_off, d_idx, gd, gb = f.RouteDevice(buf, off, rows, masks)
    assert (out.cpu().numpy().tobytes(), d_out_off.cpu().tolist(), d_idx.cpu().tolist(), gd.tolist(), gb.tolist()) == want
    f.close()


# ---- the group finder -------------------------------------------------------------------------------------------------------------
def test_group_route_json_lines():
    f = Finder(GpuEngine(), EmptyRgxEngine(), False)
    for e, t in (('"lorem"', "t0"), ('"ipsum"', "t1"), ('"dolor" and not "sit"', "t2")):
        f.AddExpressionWithTag(e, t)
    g = group.NewFinderWithRules(f, {"zeta": ['"t0"'], "alpha": ['"t1:b.c"', '"t2"'], "midé": ['"t0" and "t1"']})
    g.SetSchema(["a", "b.c", "d"])
    words = ["lorem", "ipsum", "dolor", "sit", "amet", "quux"]
    rng = np.random.default_rng(3)
    docs = []
    for i in range(50):
        pick = lambda: " ".join(rng.choice(words, 3))   # noqa: E731
        docs.append(json.dumps({"a": pick(), "b": {"c": pick()}, "d": pick()}).encode())
    docs[11] = b'{"a": "lorem", "b": {"c": '                            # a syntax error
    docs[29] = b'{"a": "lorem ipsum", "unknown": {"path": "dolor"}}'      # a path the schema does not know
    blob = b"\n".join(docs) + b"\n"
    lines = [x + b"\n" for x in docs]
    names = g.route_rule_names()
    assert names == ["alpha", "midé", "zeta"]
    parts, idx, undecided = g.RouteJsonLines(blob)
    assert undecided.tolist() == [11, 29] and len(parts) == len(idx) == 4
    assert {11, 29} <= set(idx[3].tolist()) and not {11, 29} & set(sum((i.tolist() for i in idx[:3]), []))
    results = g.ProcessJsons(lines)
    for k, name in enumerate(names):
        want = [i for i, r in enumerate(results) if i not in (11, 29) and name in r.get("rules", {})]
        assert idx[k].tolist() == want and want and parts[k] == b"".join(lines[i] for i in want), name
    want = [i for i, r in enumerate(results) if i in (11, 29) or not set(names) & set(r.get("rules", {}))]
    assert idx[3].tolist() == want and parts[3] == b"".join(lines[i] for i in want)
    first, fidx, _ = g.RouteJsonLines(blob, ["zeta", "alpha"], "first")
    assert sorted(sum((i.tolist() for i in fidx), [])) == list(range(50)) and len(first) == 3
    assert fidx[0].tolist() == idx[0].tolist() and set(fidx[1].tolist()) == set(idx[2].tolist()) - set(idx[0].tolist())
    with pytest.raises(ValueError):
        g.RouteJsonLines(blob, ["no such rule"])
