"""strings.ToLower on the device (gft_to_lower_device, csrc/gft_tolower.hip) against the host's gft_to_lower document by
document: output and offsets byte-equal, on the inputs tests/test_tolower_host.py has walked through the same piece logic on
the host; and the finder's repeat of a batch that leaves ASCII through those kernels (Finder.ProcessDevice, the
ProcessDeviceBegin / End pipeline) against the oracle over the reference-lowered text."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before libgft.so is loaded: both must share ONE HIP runtime, the one torch brings along)

from gofindthem_amd import _lib
from gofindthem_amd.engine import Engine, GftError
from gofindthem_amd.finder import EmptyRgxEngine, Finder, GpuEngine
from oracle import dsl_ref
from oracle.pyoracle import Oracle, pack_strings
from tolower_cases import edge_batches, pack, random_docs, ref_lower, reference

pytestmark = pytest.mark.gpu

GUARD = 256


@pytest.fixture(scope="module")
def eng():
    e = Engine()            # (no dictionary: the lowering needs none)
    yield e
    e.close()


def _dev(a, dtype=None):
    return torch.from_numpy(a if dtype is None else a.astype(dtype)).cuda()


def lower(eng, docs, lead=0, cap=None):
    """count only, then a second call with `cap` (default: the total) -> (out [cap + GUARD] bytes, out_off, total)"""
    blob, off = pack(docs, lead)
    t, o = _dev(blob), _dev(off, np.int64)
    out_off = torch.full((len(docs) + 1,), 0x5A5A, dtype=torch.int64, device="cuda")
    total = eng.to_lower_device(t.data_ptr(), o.data_ptr(), len(docs), None, 0, out_off.data_ptr())
    counted = out_off.cpu().numpy().astype(np.uint64)
    if cap is None:
        cap = total
    out = torch.full((cap + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    out_off.fill_(0x5A5A)
    assert eng.to_lower_device(t.data_ptr(), o.data_ptr(), len(docs), out.data_ptr(), cap, out_off.data_ptr()) == total
    got_off = out_off.cpu().numpy().astype(np.uint64)
    assert np.array_equal(counted, got_off), "the count-only call and the writing call disagree on the offsets"
    return out.cpu().numpy().tobytes(), got_off, total, cap


def check(eng, docs, lead=0):
    want, want_off = reference(docs)
    out, off, total, cap = lower(eng, docs, lead)
    assert total == len(want)
    assert np.array_equal(off, want_off)
    if out[:cap] != want:
        i = next(i for i in range(len(want)) if out[i] != want[i])
        d = int(np.searchsorted(want_off, i, side="right")) - 1
        raise AssertionError("byte %d (document %d, byte %d of its lower-case form) differs" % (i, d, i - int(want_off[d])))
    assert out[cap:] == b"\xa5" * GUARD, "bytes stored past cap"


@pytest.mark.parametrize("name", sorted(edge_batches()))
def test_edge_inputs(eng, name):
    docs = edge_batches()[name]
    check(eng, docs)
    check(eng, docs, lead=5)              # doc_off[0] != 0, in front of it a byte that would lead the first document's


def test_no_documents(eng):
    out_off = torch.full((1,), 77, dtype=torch.int64, device="cuda")
    assert eng.to_lower_device(None, None, 0, None, 0, out_off.data_ptr()) == 0
    assert out_off.cpu().tolist() == [0]
    off = _dev(np.array([9], np.int64))
    assert eng.to_lower_device(None, off.data_ptr(), 0, None, 0, out_off.data_ptr()) == 0


def test_random_family(eng):
    check(eng, random_docs())


def test_cap_below_the_total(eng):
    docs = edge_batches()["length_changers"] + edge_batches()["invalid"] + [b"plain ASCII " * 40] + random_docs(200, seed=5)
    want, want_off = reference(docs)
    for cap in (len(want) - 1, len(want) - 17, len(want) // 2):
        out, off, total, _ = lower(eng, docs, cap=cap)
        assert total == len(want) and np.array_equal(off, want_off)
        assert out[:cap] == want[:cap]
        assert out[cap:] == b"\xa5" * GUARD, "cap %d: bytes stored past cap" % cap


def test_refusals_leave_the_handle_usable(eng):
    blob, off = pack([b"abc", b"DEF\xc3\x89"])
    t = _dev(blob)
    out = torch.zeros(64, dtype=torch.uint8, device="cuda")
    out_off = torch.zeros(3, dtype=torch.int64, device="cuda")
    desc = _dev(np.array([0, 5, 3], np.int64))
    o = _dev(off, np.int64)
    for args in ((t.data_ptr(), desc.data_ptr(), 2, out.data_ptr(), 64, out_off.data_ptr()),          # offsets descend
                 (t.data_ptr(), o.data_ptr(), 2, t.data_ptr() + 4, 16, out_off.data_ptr()),            # output inside the input
                 (t.data_ptr(), o.data_ptr(), 2, out.data_ptr(), 64, o.data_ptr()),                    # offsets on the input's
                 (t.data_ptr(), o.data_ptr(), 2, None, 8, out_off.data_ptr())):                        # cap without a buffer
        with pytest.raises(GftError) as ei:
            eng.to_lower_device(*args)
        assert ei.value.code == _lib.GFT_E_INVALID
    assert t.cpu().numpy()[:8].tobytes() == b"abcDEF\xc3\x89" and o.cpu().tolist() == [0, 3, 8]
    assert eng.to_lower_device(t.data_ptr(), o.data_ptr(), 2, out.data_ptr(), 64, out_off.data_ptr()) == 8
    assert out.cpu().numpy()[:8].tobytes() == "abcdefé".encode() and out_off.cpu().tolist() == [0, 3, 8]


def test_profile_names_and_the_verdict_is_left_alone(eng):
    L = _lib.load()
    before = L.gft_last_nonascii(eng._h)
    eng.profile(True)
    eng.profile_reset()
    check(eng, [b"\xc3\x89COLE " * 300, b"ascii"])
    for name in ("lower_count", "lower_scan", "lower_write"):
        ms, n = eng.profile_read(name)
        assert n == (1 if name == "lower_write" else 2) and ms > 0, name       # (check() counts, then counts and writes)
    eng.profile(False)
    assert L.gft_last_nonascii(eng._h) == before


def test_handles_over_several_devices_are_refused():
    e = Engine(devices=[0, 0])
    out_off = torch.zeros(1, dtype=torch.int64, device="cuda")
    with pytest.raises(GftError) as ei:
        e.to_lower_device(None, None, 0, None, 0, out_off.data_ptr())
    assert ei.value.code == _lib.GFT_E_UNSUPPORTED
    e.close()


# ---- the finder -------------------------------------------------------------------------------------------------------------
EXPRS = ['"école"', '"ecole" or "straße"', '"la" and not "k"', 'inord("la" and "carte")', '"kelvin"', '"istanbul"', '"�"',
         'inord("273" and "kelvin")']
UPPER = ["Vive la École", "LA STRASSE École", "la carte", "k", "273 Kelvin", "İstanbul", b"caf\xff\xc3 LA CARTE \xe2\x82"]
ASCII = ["ECOLE la", "k LA carte", "plain text", "la CARTE ecole"]
LATIN1 = ["vive la école", "LA STRAßE", "à la carte", "plain ECOLE"]


def _keywords(exprs):
    kw = {}
    for e in exprs:
        kw.update(dict.fromkeys(dsl_ref.parse(e, False)[1]))
    return sorted(kw)


@pytest.fixture(scope="module")
def oracle():
    o = Oracle(_keywords(EXPRS))
    o.set_expressions(EXPRS, False)
    return o


def _batch(texts, n, shift, oracle):
    docs = [texts[(d + shift) % len(texts)] for d in range(n)]
    docs = [d.encode("utf-8") if isinstance(d, str) else d for d in docs]
    lb, lo = pack_strings([ref_lower(d) for d in docs])
    want = oracle.process(lb, lo, fold=False)
    blob, off = pack(docs)
    return _dev(blob), _dev(off, np.int64), n, want


def _run_finder(oracle):
    """synchronous batches, then the pipeline with a younger batch in flight -> (bitmaps as arrays, lowered_batches())"""
    f = Finder(GpuEngine(), EmptyRgxEngine(), False)
    f.AddExpressions(EXPRS)
    words = (len(EXPRS) + 31) // 32
    got = []
    plain = [_batch(ASCII, 150, 0, oracle), _batch(LATIN1, 150, 1, oracle)]
    for t, o, n, want in plain * 2:
        bm = torch.zeros((n, words), dtype=torch.int32, device="cuda")
        f.ProcessDevice(t.data_ptr(), o.data_ptr(), n, bm.data_ptr())
        assert np.array_equal(bm.cpu().numpy().astype(np.uint32), want)
    assert f.lowered_batches() == (0, 0), "ASCII and lower-case Latin-1 batches were repeated"
    up = _batch(UPPER, 210, 0, oracle)
    needs_tolower = 0b11110001          # école, kelvin, istanbul, U+FFFD, inord(273, kelvin): true only after strings.ToLower
    assert int(np.bitwise_or.reduce(up[3][:, 0])) & needs_tolower == needs_tolower
    bm = torch.zeros((up[2], words), dtype=torch.int32, device="cuda")
    f.ProcessDevice(up[0].data_ptr(), up[1].data_ptr(), up[2], bm.data_ptr())
    got.append(bm.cpu().numpy().astype(np.uint32))
    assert np.array_equal(got[-1], up[3]), "ProcessDevice"
    sync_counts = f.lowered_batches()
    # the pipeline: always one batch begun ahead of the one that ends
    seq = [_batch(UPPER, 200, 1, oracle), plain[0], _batch(UPPER, 200, 2, oracle), _batch(UPPER, 200, 3, oracle), plain[1]]
    bms = [torch.zeros((200, words), dtype=torch.int32, device="cuda") for _ in range(2)]
    begun = []

    def end_oldest():
        i, slot = begun.pop(0)
        f.ProcessDeviceEnd()
        g = bms[slot].cpu().numpy().astype(np.uint32)[:seq[i][2]]
        assert np.array_equal(g, seq[i][3]), "pipelined batch %d" % i
        got.append(g)

    for i, b in enumerate(seq):
        slot = i % 2
        if any(s == slot for _, s in begun):
            end_oldest()
        bms[slot].zero_()
        f.ProcessDeviceBegin(b[0].data_ptr(), b[1].data_ptr(), b[2], bms[slot].data_ptr())
        begun.append((i, slot))
        while len(begun) > 1:
            end_oldest()
    while begun:
        end_oldest()
    counts = f.lowered_batches()
    f.close()
    return got, sync_counts, counts


def test_finder_repeats_on_the_device(oracle, monkeypatch):
    monkeypatch.delenv("GFT_DEVICE_TOLOWER", raising=False)
    got_dev, sync_dev, all_dev = _run_finder(oracle)
    assert sync_dev == (1, 0) and all_dev == (4, 0), "the device path was not taken for every batch that left ASCII"
    monkeypatch.setenv("GFT_DEVICE_TOLOWER", "0")
    got_host, sync_host, all_host = _run_finder(oracle)
    assert sync_host == (0, 1) and all_host == (0, 4), "GFT_DEVICE_TOLOWER=0 did not keep the host path"
    assert len(got_dev) == len(got_host) and all(np.array_equal(a, b) for a, b in zip(got_dev, got_host))
