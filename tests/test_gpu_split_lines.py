"""A blob cut into line documents on the device (csrc/gft_split.hip): Engine.split_lines_device against the reference of
split_lines.py on every fixed and random case in both modes, at unaligned bases and with the slack bytes filled two ways; the cap
protocol; the refusals; one blob past 4 GiB; and the callers -- Finder.ProcessLinesDevice / ProcessLines against ProcessTexts over
the pieces, GroupFinder.ProcessJsonLinesDevice / ProcessJsonLines against the calls that take the documents as a list."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before libgft.so is loaded: one HIP runtime)

import json_docs as J
import records as R
import split_lines as S
from gofindthem_amd import _lib, group
from gofindthem_amd.engine import Engine, GftError, split_shape
from gofindthem_amd.finder import EmptyRgxEngine, Finder, FinderError, GpuEngine, PyRegexpEngine
from gofindthem_amd.workload import Workload

pytestmark = pytest.mark.gpu

MODES = [S.AFTER_NL, S.JSON_LINES]
GUARD = -0x5A5A5A5A5A5A5A5B


@pytest.fixture(scope="module")
def eng():
    e = Engine()
    yield e
    e.close()


def resident(blob, at=0, fill=0):
    """the blob at byte `at` of an allocation whose other bytes -- the 64 of slack among them -- hold `fill`"""
    buf = torch.full((at + len(blob) + 64 + 16,), fill, dtype=torch.uint8, device="cuda")
    if blob:
        buf[at:at + len(blob)] = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    return buf[at:]


def split(eng, blob, mode, at=0, fill=0):
    return eng.split_lines_device(resident(blob, at, fill), len(blob), mode).cpu().tolist()


@pytest.mark.parametrize("mode", MODES)
def test_fixed_cases(eng, mode):
    want = S.expected("fixed")
    for name, blob in S.fixed_cases():
        assert split(eng, blob, mode) == want[name, mode], name


@pytest.mark.parametrize("fill", [10, ord("{")], ids=["newlines behind", "braces behind"])
@pytest.mark.parametrize("mode", MODES)
def test_unaligned_bases_and_what_the_slack_holds(eng, mode, fill):
    want = S.expected("fixed")
    for name, blob in S.fixed_cases():
        for at in (1, 3, 8, 15):
            assert split(eng, blob, mode, at, fill) == want[name, mode], (name, at)


@pytest.mark.parametrize("mode", MODES)
def test_random_blobs(eng, mode):
    want = S.expected("random")
    for name, blob in S.random_cases():
        assert split(eng, blob, mode, fill=ord("a")) == want[name, mode], name


def raw_split(eng, buf, length, mode, cap, guard=4):
    """gft_split_lines_device into a tensor of cap + guard entries -> (n, the tensor on the host)"""
    L = _lib.load()
    off = torch.full((cap + guard,), GUARD, dtype=torch.int64, device="cuda")
    n = C.c_uint64(99)
    torch.cuda.synchronize()
    eng._check(L.gft_split_lines_device(eng._h, buf.data_ptr(), length, mode, off.data_ptr() if cap else None, cap, C.byref(n)))
    return int(n.value), off.cpu().numpy()


@pytest.mark.parametrize("mode", MODES)
def test_cap_protocol(eng, mode):
    T, _ = split_shape()
    blob = S.short_lines(3 * T + 11, 5)
    want = S.reference(blob, mode)
    n = len(want) - 1
    buf = resident(blob)
    assert raw_split(eng, buf, len(blob), mode, 0)[0] == n                       # count only
    got, off = raw_split(eng, buf, len(blob), mode, n + 1)
    assert got == n and off[:n + 1].tolist() == want and (off[n + 1:] == GUARD).all()
    for cap in (n, n // 2, 1):                                                   # entries at and past cap are not written
        got, off = raw_split(eng, buf, len(blob), mode, cap)
        assert got == n and off[:cap].tolist() == want[:cap] and (off[cap:] == GUARD).all(), cap
    got, off = raw_split(eng, resident(b" \n\t"), 3, S.JSON_LINES, 3)             # no document: entry 0 alone
    assert got == 0 and off[0] == 0 and (off[1:] == GUARD).all()
    got, off = raw_split(eng, resident(b""), 0, mode, 2)
    assert got == 0 and off[0] == 0 and (off[1:] == GUARD).all()


def test_refusals_leave_the_handle_usable(eng):
    L = _lib.load()
    buf = resident(b"ab\ncd\n")
    n = C.c_uint64(0)
    off = torch.zeros(8, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert L.gft_split_lines_device(eng._h, buf.data_ptr(), 6, 2, off.data_ptr(), 8, C.byref(n)) == _lib.GFT_E_INVALID      # unknown mode
    assert L.gft_split_lines_device(eng._h, buf.data_ptr(), 6, 0, None, 8, C.byref(n)) == _lib.GFT_E_INVALID                # a cap, no array
    assert L.gft_split_lines_device(eng._h, None, 6, 0, off.data_ptr(), 8, C.byref(n)) == _lib.GFT_E_INVALID
    both = torch.zeros(256, dtype=torch.uint8, device="cuda")                                                               # output over the slack
    assert L.gft_split_lines_device(eng._h, both.data_ptr(), 64, 0, both.data_ptr() + 120, 4, C.byref(n)) == _lib.GFT_E_INVALID
    with pytest.raises(ValueError):
        eng.split_lines_device(torch.zeros(10, dtype=torch.uint8, device="cuda"), 10, 0)                                    # no slack
    assert eng.split_lines_device(buf, 6, 0).cpu().tolist() == [0, 3, 6]


def test_profile_names_and_the_verdict_is_left_alone(eng):
    L = _lib.load()
    before = L.gft_last_nonascii(eng._h)
    eng.profile(True)
    eng.profile_reset()
    blob = "é\nÉ\n".encode("utf-8") * 1000
    assert eng.split_lines_device(resident(blob), len(blob), S.JSON_LINES).numel() == 2001
    for name in ("split_count", "split_scan", "split_write"):
        ms, k = eng.profile_read(name)
        assert k >= 1 and ms >= 0, name
    eng.profile(False)
    assert L.gft_last_nonascii(eng._h) == before


def test_handles_over_several_devices_are_refused():
    e = Engine(devices=[0, 0])
    buf = resident(b"ab\ncd\n")
    with pytest.raises(GftError) as ei:
        e.split_lines_device(buf, 6, 0)
    assert ei.value.code == _lib.GFT_E_UNSUPPORTED
    e.close()
    one = Engine()
    assert one.split_lines_device(buf, 6, 0).cpu().tolist() == [0, 3, 6]
    one.close()


@pytest.mark.parametrize("mode", MODES)
def test_a_blob_past_four_gib(eng, mode):
    """the smallest shape at which a 32-bit offset or tile index shows: 2^32 + 2 T spaces with a handful of bytes planted on both
    sides of 2^32 and across it"""
    T, _ = split_shape()
    G = 1 << 32
    length = G + 2 * T
    buf = torch.full((length + 64,), 32, dtype=torch.uint8, device="cuda")
    planted = {5: 10, 9: ord("{"), T + 3: 10, G - T - 1: ord("{"), G - 2: 10, G - 1: ord("{"), G: 10, G + 1: 10, G + 7: ord("{"), G + T: 10,
               G + T + 1: ord("{"), length - 1: 10}
    pos = torch.tensor(sorted(planted), dtype=torch.int64, device="cuda")
    buf[pos] = torch.tensor([planted[p] for p in sorted(planted)], dtype=torch.uint8, device="cuda")
    want = S.sparse_reference(length, planted, mode)
    assert max(want[1:-1]) > G and len(want) > 4
    assert eng.split_lines_device(buf, length, mode).cpu().tolist() == want
    del buf
    torch.cuda.empty_cache()


# ---- the finder -----------------------------------------------------------------------------------------------------------------
def test_finder_process_lines():
    w = Workload(300)
    text, off = w.docs_host(0, 300)
    docs = [bytes(text[int(off[i]):int(off[i + 1])]).replace(b"\n", b" ") for i in range(300)]
    terms = [t.decode("ascii") for t in w.terms() if t.isalpha()][:40]
    docs[7] = b""                                                      # an empty line
    docs[11] = docs[11] + b" " + terms[0].encode()                     # a keyword in front of its line's newline
    docs[20] = ("VIVE LA École " + terms[1].upper()).encode("utf-8")   # leaves ASCII: lowered on the device, scanned again
    blob = b"\n".join(docs)                                            # (no final newline: the last piece has none)
    f = Finder(GpuEngine(), EmptyRgxEngine(), False)
    f.AddExpressions(['"%s"' % t for t in terms[:20]] + ['"%s\n"' % terms[0], '"école" and "%s"' % terms[1],
                                                         '"%s" and not "%s"' % (terms[2], terms[3])])
    pieces = S.documents(blob, S.AFTER_NL)
    assert len(pieces) == 300 and pieces[7] == b"\n" and pieces[-1][-1:] != b"\n"
    want = f.ProcessTexts(pieces)
    col = 20
    assert want[11, col // 32] >> (col % 32) & 1 and want[20, (col + 1) // 32] >> ((col + 1) % 32) & 1 and want.any(axis=1).sum() > 50
    before = f.lowered_batches()
    d_off, d_rows = f.ProcessLinesDevice(resident(blob), len(blob))
    assert f.lowered_batches() == (before[0] + 1, before[1])
    assert d_off.cpu().tolist() == S.reference(blob, S.AFTER_NL)
    assert np.array_equal(d_rows.cpu().numpy().view(np.uint32), want)
    h_off, h_rows = f.ProcessLines(blob)
    assert h_off.tolist() == S.reference(blob, S.AFTER_NL) and np.array_equal(h_rows, want)
    h_off, h_rows = f.ProcessLines(b"")
    assert h_off.tolist() == [0] and h_rows.shape == (0, want.shape[1])


def test_finder_process_lines_needs_what_process_device_needs():
    f = Finder(GpuEngine(), PyRegexpEngine(), False)
    f.AddExpressions(['"ab"', 'r"a+b"'])
    buf = resident(b"ab\ncd\n")
    with pytest.raises(FinderError) as e1:
        f.ProcessLinesDevice(buf, 6)
    off = torch.tensor([0, 3, 6], dtype=torch.int64, device="cuda")
    rows = torch.zeros((2, 1), dtype=torch.int32, device="cuda")
    with pytest.raises(FinderError) as e2:
        f.ProcessDevice(buf.data_ptr(), off.data_ptr(), 2, rows.data_ptr())
    assert e1.value.code == e2.value.code == _lib.GFT_E_UNSUPPORTED and str(e1.value) == str(e2.value)


# ---- the group finder -------------------------------------------------------------------------------------------------------------
def make_group(seed, schema=None):
    rng = np.random.default_rng(seed)
    paths = R.make_schema(8)
    exprs, tags = R.make_expressions(40, 5, rng)
    f = Finder(GpuEngine(), EmptyRgxEngine(), False)
    for e, t in zip(exprs, tags):
        f.AddExpressionWithTag(e, t)
    g = group.NewFinderWithRules(f, R.make_rules(20, 5, paths, rng))
    if schema:
        g.SetSchema(paths)
    return g, paths, rng


def json_lines(paths, rng, n=200):
    """n generated documents, a line each, joined by a mix of line ends, blank lines and indentation; one malformed line and one
    document the device hands to the host (a surrogate escape at a schema path)"""
    docs = [J.gen_doc(paths, rng, R.vocabulary()).replace(b"\n", b" ").replace(b"\r", b" ") for _ in range(n)]
    docs[n // 3] = b'{"%s": ' % paths[0].encode()
    docs[n // 2] = b'{"%s":"\\ud800 %s"}' % (paths[0].encode(), R.vocabulary()[0].encode())
    ends = [b"\n", b"\r\n", b"\n\n", b"\n \t\r\n", b"\r\n\r\n"]
    indents = [b"", b"", b"  ", b"\t "]
    parts = [b"\n \n"]
    for d in docs:
        parts += [indents[int(rng.integers(len(indents)))], d, ends[int(rng.integers(len(ends)))]]
    blob = b"".join(parts)[:-1] if rng.integers(2) else b"".join(parts)
    lines = S.documents(blob, S.JSON_LINES)
    assert len(lines) == n and b"".join(lines) == blob
    return blob, lines


def test_process_json_lines_with_a_schema():
    g, paths, rng = make_group(11, schema=True)
    blob, lines = json_lines(paths, rng)
    want = g.ProcessJsonsSchema(lines)
    assert g.ProcessJsonLines(blob) == want
    n_device, n_host = g.json_last()
    assert n_device + n_host == 200 and n_host >= 2 and n_device > 150
    assert "error" in want[200 // 3] and 20 < sum(1 for r in want if r.get("rules"))
    with pytest.raises(group.GroupFinderError) as e:
        g.ProcessJsonLines(blob, [paths[0]], None)
    assert e.value.code == _lib.GFT_E_INVALID
    assert g.ProcessJsonLines(b" \n\n") == [] and g.ProcessJsonLines(blob) == want


def test_process_json_lines_without_a_schema():
    g, paths, rng = make_group(12)
    blob, lines = json_lines(paths, rng)
    inc, exc = [paths[0], paths[5]], [paths[2]]
    want = g.ProcessJsonsAuto(lines, inc, exc)
    assert g.ProcessJsonLines(blob, inc, exc) == want
    assert sum(g.json_last()) == 200 and g.json_last()[0] > 150
    assert g.ProcessJsonLines(blob) == g.ProcessJsonsAuto(lines)
    assert "error" in want[200 // 3]


def test_process_json_lines_device():
    g, paths, rng = make_group(13, schema=True)
    blob, lines = json_lines(paths, rng)
    buf = resident(blob, fill=ord("{"))
    off, rows, status = g.ProcessJsonLinesDevice(buf, len(blob))
    assert off.cpu().tolist() == S.reference(blob, S.JSON_LINES)
    want_rows, want_status = g.ProcessJsonsDevice(*J.to_device(lines))
    assert torch.equal(status.cpu(), want_status.cpu()) and torch.equal(rows.cpu(), want_rows.cpu())
    leaves_status = g.JsonLeavesDevice(buf, off)[0]
    assert torch.equal(status.cpu(), leaves_status.cpu())
    st = status.cpu().tolist()
    assert st[200 // 3] == J.SYNTAX and st[200 // 2] == J.TEXT and st.count(0) > 150
    # the tag side takes the same offsets as they are
    ent, tag_status = g.TagJsonsDevice(buf, off)
    assert torch.equal(tag_status.cpu(), status.cpu())
    g2, _, _ = make_group(13)
    with pytest.raises(group.GroupFinderError):
        g2.ProcessJsonLinesDevice(buf, len(blob))                      # a schema must be set
