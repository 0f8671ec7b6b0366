"""What a batch reports back, on the host (no GPU): csrc/batch_verdict.cpp through gft_debug_judge_batch / gft_debug_learn.

The hooks decode a forged control-block read-back and judge it against a forged launch record with the functions that
gft_process_device and gft_process_device_end call, and run the function that turns a completed batch into the next
batches' unit size and match density.  The GPU suite (tests/test_gpu_pipeline.py) keeps the checks that real batches in
flight are judged so; here every branch of the judgement is pinned by itself, in the order the checks are made.
"""
import ctypes as C

import pytest

from gofindthem_amd import _lib

ACCEPT, AGAIN_GENERAL, AGAIN_GROW, INVALID = 0, 1, 2, 3
UNIT_MAX = 8192                  # kScan2UnitMax
FIFO = 256                       # kScan2FifoCap


def ctl(bad=0, cursor=0, total=0, bits=0, miss=0, n_units=0, lo=0, hi=0, bad_high=0):
    """the seven words of a read-back (csrc/batch_verdict.hpp): word 0 = bad-offsets flag (u32), 1 = cursor, 2 = match
    count, 3 = non-ASCII bits (low half) and the single-unit-miss epoch (high half), 4 .. 6 = n_units, text_lo, text_hi"""
    return [bad | bad_high << 32, cursor, total, bits | miss << 32, n_units, lo, hi]


def judge(words, single=False, epoch=0, n_docs=100, unit_cap=100, pool_cap=1 << 20, static_slabs=0):
    """-> (kind, pool_need, verdict dict, error text)"""
    L = _lib.load()
    w = (C.c_uint64 * 7)(*words)
    kind, need, v, err = C.c_int(-1), C.c_uint64(0), (C.c_uint64 * 6)(), C.create_string_buffer(256)
    rc = L.gft_debug_judge_batch(C.addressof(w), int(single), epoch, n_docs, unit_cap, pool_cap, static_slabs, C.byref(kind),
                                 C.byref(need), C.addressof(v), C.addressof(err), len(err))
    assert rc == 0
    verdict = dict(zip(("nonascii", "bits", "text_lo", "text_hi", "n_units", "total"), list(v)))
    return kind.value, need.value, verdict, err.value.decode()


GOOD = dict(total=777, n_units=100, lo=64, hi=5000)
GOOD_VERDICT = dict(nonascii=0, bits=0, text_lo=64, text_hi=5000, n_units=100, total=777)
SLABS = 3 * 4096                 # what the waves of a grid owned from the start: the cursor counts behind them
POOL = 1 << 20


def test_cursor_at_the_end_of_the_launch_pool_is_accepted_one_above_is_not():
    at = POOL - SLABS
    assert judge(ctl(cursor=at, **GOOD), pool_cap=POOL, static_slabs=SLABS) == (ACCEPT, 0, GOOD_VERDICT, "")
    c = at + 1 + SLABS           # the full cursor
    assert judge(ctl(cursor=at + 1, **GOOD), pool_cap=POOL, static_slabs=SLABS) == (AGAIN_GROW, c + c // 16, GOOD_VERDICT, "")
    # the DFA kernel owns nothing: its cursor alone is judged
    assert judge(ctl(cursor=POOL, **GOOD), pool_cap=POOL)[0] == ACCEPT
    assert judge(ctl(cursor=POOL + 1, **GOOD), pool_cap=POOL)[:2] == (AGAIN_GROW, POOL + 1 + (POOL + 1) // 16)


def test_unit_table_exactly_full_is_accepted_one_more_is_not():
    assert judge(ctl(cursor=5, **dict(GOOD, n_units=250)), unit_cap=250)[:2] == (ACCEPT, 0)
    kind, need, v, _ = judge(ctl(cursor=5, **dict(GOOD, n_units=251)), unit_cap=250)
    assert (kind, need) == (AGAIN_GENERAL, 0) and v["n_units"] == 251
    # both outgrown: the pool is grown for the second run
    assert judge(ctl(cursor=POOL + 1, **dict(GOOD, n_units=251)), unit_cap=250, pool_cap=POOL)[0] == AGAIN_GROW


def test_only_the_pool_of_the_launch_counts():
    """a launch with a small pool: whatever the engine's pool has grown to since (another batch's rerun, a younger batch
    that sized it from its text), the kernels of THIS launch wrote nothing beyond pool_cap -- the function is given no
    other size to look at, and says again"""
    c = 70_000
    assert judge(ctl(cursor=c, **GOOD), pool_cap=65_536) == (AGAIN_GROW, c + c // 16, GOOD_VERDICT, "")
    assert judge(ctl(cursor=c - SLABS, **GOOD), pool_cap=65_536, static_slabs=SLABS)[:2] == (AGAIN_GROW, c + c // 16)


def test_single_unit_launch_reads_its_flags_by_epoch():
    # word 0 holds what an OLDER batch raised it to: not this batch's business
    assert judge(ctl(bad=6, cursor=5, **GOOD), single=True, epoch=7) == (ACCEPT, 0, GOOD_VERDICT, "")
    kind, _, _, err = judge(ctl(bad=7, cursor=5, **GOOD), single=True, epoch=7)
    assert kind == INVALID and "4 GiB" in err
    # the miss flag likewise
    assert judge(ctl(miss=6, cursor=5, **GOOD), single=True, epoch=7)[0] == ACCEPT
    assert judge(ctl(miss=7, cursor=5, **GOOD), single=True, epoch=7)[:2] == (AGAIN_GENERAL, 0)


def test_single_unit_miss_comes_before_every_other_check():
    """a document of more than one unit under the one-launch unit table: the batch goes the general way, whatever else the
    block says -- a descending range, a raised flag, a cursor past the pool"""
    for extra in (dict(lo=9, hi=3), dict(bad=7), dict(cursor=POOL + 1), dict(lo=9, hi=3, bad=7, cursor=POOL + 1)):
        kind, need, v, err = judge(ctl(**dict(dict(GOOD, bits=1), miss=7, **extra)), single=True, epoch=7, pool_cap=POOL)
        assert (kind, need, err) == (AGAIN_GENERAL, 0, ""), extra
        assert (v["bits"], v["nonascii"]) == (1, 1)
    # a general launch never reads that half of word 3
    assert judge(ctl(miss=7, cursor=5, **GOOD), epoch=7)[0] == ACCEPT


def test_general_launch_takes_any_raised_flag():
    for bad in (1, 6, 0xFFFFFFFF):
        kind, _, v, err = judge(ctl(bad=bad, cursor=5, **GOOD))
        assert kind == INVALID and "4 GiB" in err and v == GOOD_VERDICT
    # (the flag is the low half of word 0)
    assert judge(ctl(bad_high=1, cursor=5, **GOOD))[0] == ACCEPT


def test_descending_text_range():
    kind, need, _, err = judge(ctl(cursor=5, **dict(GOOD, lo=5000, hi=4999)))
    assert (kind, need, err) == (INVALID, 0, "doc_off is not ascending")
    # ... is judged before the flag, and both before the sizes
    assert judge(ctl(bad=1, cursor=POOL + 1, **dict(GOOD, lo=5000, hi=4999)), pool_cap=POOL)[3] == "doc_off is not ascending"
    assert judge(ctl(bad=1, cursor=POOL + 1, **GOOD), pool_cap=POOL)[0] == INVALID
    assert judge(ctl(cursor=5, **dict(GOOD, lo=5000, hi=5000)))[0] == ACCEPT          # (an empty range is a range)


@pytest.mark.parametrize("bits", [0, 1, 2, 3])
def test_nonascii_bits_are_copied_through(bits):
    _, _, v, _ = judge(ctl(cursor=5, bits=bits, **GOOD))
    assert v == dict(GOOD_VERDICT, bits=bits, nonascii=int(bits != 0))
    _, _, v, _ = judge(ctl(cursor=POOL + 1, bits=bits, **GOOD), pool_cap=POOL)
    assert (v["bits"], v["nonascii"]) == (bits, int(bits != 0))


# ---- what a completed batch teaches the next ones ------------------------------------------------------------------------
def learn(kernel, total, lo, hi, fifo_cap=FIFO, ordered=False, unit_max=UNIT_MAX, density=0.06):
    L = _lib.load()
    um, d = C.c_uint32(unit_max), C.c_double(density)
    assert L.gft_debug_learn(kernel.encode(), fifo_cap, int(ordered), total, lo, hi, C.byref(um), C.byref(d)) == 0
    return um.value, d.value


def test_learn_unit_size_from_the_match_density():
    """unit_max = 0.75 x fifo_cap / (matches per byte), rounded down to a multiple of 256, within [512, 8192]"""
    # dense: 1000 matches in 8000 bytes = 0.125 per byte -> 192 / 0.125 = 1536
    assert learn("scan5", 1000, 100, 8100) == (1536, 0.06)
    assert learn("scan2", 1000, 100, 8100) == (1536, 0.06)
    # ... with a fifo of 512 entries: 384 / 0.125 = 3072
    assert learn("scan5", 1000, 100, 8100, fifo_cap=512) == (3072, 0.06)
    # sparse: 1000 matches in 32000 bytes = 1 / 32 per byte -> 192 * 32 = 6144; in 33000 bytes: 6336 -> 6144 too
    assert learn("scan5", 1000, 0, 32000, unit_max=1536) == (6144, 0.06)
    assert learn("scan5", 1000, 0, 33000, unit_max=1536) == (6144, 0.06)
    # floor: two matches per byte -> 96 -> 0 -> 512
    assert learn("scan5", 16000, 0, 8000) == (512, 0.06)
    # ceiling: 192 / (1 / 1000) = 192 000; and no match at all
    assert learn("scan5", 8, 0, 8000, unit_max=512) == (UNIT_MAX, 0.06)
    assert learn("scan5", 0, 0, 8000, unit_max=512) == (UNIT_MAX, 0.06)


def test_learn_leaves_alone_what_it_must():
    # an empty or descending range teaches nothing
    for lo, hi in ((500, 500), (500, 499)):
        assert learn("scan4", 1000, lo, hi, unit_max=1024, density=0.5) == (1024, 0.5)
    # every unit through the per-lane staging path (GFT_SCAN_ORDERED): the fifo was not used, the unit size stays
    assert learn("scan5", 1000, 100, 8100, ordered=True) == (UNIT_MAX, 0.06)
    assert learn("scan4", 1000, 100, 8100, ordered=True) == (UNIT_MAX, 0.125)
    # the kernels with a unit size of their own
    for k in ("dfa", "scan3"):
        assert learn(k, 1000, 100, 8100, unit_max=1024, density=0.5) == (1024, 0.5)


def test_learn_scan4_density():
    assert learn("scan4", 1000, 100, 8100) == (1536, 0.125)
    assert learn("scan4", 1, 0, 8000) == (UNIT_MAX, 0.002)                # floor: 1 / 8000 per byte
    assert learn("scan4", 0, 0, 8000) == (UNIT_MAX, 0.002)
    assert learn("scan5", 1000, 100, 8100, density=0.5)[1] == 0.5         # (scan4's alone)
