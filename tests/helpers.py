"""Shared test helpers (test infrastructure)."""
import ctypes as C

import numpy as np

from oracle import dsl_ref
from oracle.pyoracle import pack_strings

OP_UNIT, OP_AND, OP_OR, OP_NOT, OP_INORD = 1, 2, 3, 4, 5
INORD_FLAG = 1 << 27


def tree_to_program(e, slot_of):
    """dsl_ref.Expression -> postfix uint32 words of include/gft.h (independent of the product's own
    compiler in csrc/dsl_compile.cpp, so the two can be checked against each other)."""
    out = []

    def walk(n):
        fl = INORD_FLAG if n.Inord else 0
        if n.Type == dsl_ref.UNIT_EXPR:
            out.append(OP_UNIT << 28 | fl | slot_of(n.Literal))
        elif n.Type in (dsl_ref.AND_EXPR, dsl_ref.OR_EXPR):
            walk(n.LExpr)
            walk(n.RExpr)
            out.append((OP_AND if n.Type == dsl_ref.AND_EXPR else OP_OR) << 28 | fl)
        elif n.Type == dsl_ref.NOT_EXPR:
            walk(n.RExpr)
            out.append(OP_NOT << 28)
        elif n.Type == dsl_ref.INORD_EXPR:
            walk(n.RExpr)
            out.append(OP_INORD << 28)
        else:
            raise ValueError("unexpected node type %d" % n.Type)

    walk(e)
    return out


def docs(texts):
    return pack_strings(texts)


def csr_lists(moff, tid, pos):
    return [list(zip(tid[int(moff[d]):int(moff[d + 1])].tolist(), pos[int(moff[d]):int(moff[d + 1])].tolist()))
            for d in range(len(moff) - 1)]


def assert_csr_equal(a, b):
    for x, y, name in zip(a, b, ("match_off", "term_id", "pos")):
        assert x.shape == y.shape, (name, x.shape, y.shape)
        if not np.array_equal(x, y):
            bad = np.nonzero(x != y)[0][:5]
            raise AssertionError("%s differs at %s: %s vs %s" % (name, bad, x[bad], y[bad]))


# ---- the table set and the scan plan on the host (gft_debug_tables, gft_debug_scan_plan, gft_debug_learn) -----------------
LDS_GFX950 = 160 * 1024          # what gft_engine_create sets on gfx950


class Refused(Exception):
    def __init__(self, code, msg):
        super().__init__("gft error %d: %s" % (code, msg))
        self.code = code


def tables(terms=None, blob=None, forced="auto", lds_max=LDS_GFX950):
    """-> (chosen kernel's name, written blob); Refused with the status and the text of a refusal"""
    from gofindthem_amd import _lib
    L = _lib.load()
    tb, to = pack_strings(terms or [])
    kernel, needed, err = C.c_char_p(), C.c_uint64(0), C.create_string_buffer(512)
    out = C.create_string_buffer(4 << 20)
    for _ in range(2):
        rc = L.gft_debug_tables(tb.ctypes.data, to.ctypes.data, len(terms or []), blob, len(blob) if blob is not None else 0, lds_max,
                                forced.encode() if forced is not None else None, C.byref(kernel), C.addressof(out), len(out),
                                C.byref(needed), C.addressof(err), len(err))
        if rc == _lib.GFT_E_INVALID and needed.value > len(out):
            out = C.create_string_buffer(needed.value)
            continue
        break
    if rc:
        raise Refused(rc, err.value.decode())
    return kernel.value.decode(), out.raw[:needed.value]


def scan_plan(terms, forced="auto", lds_max=LDS_GFX950):
    """-> (kernel, dict of plan_scan's numbers for `terms`: gft_debug_scan_plan)"""
    from gofindthem_amd import _lib
    tb, to = pack_strings(terms)
    kernel, plan = C.c_char_p(), (C.c_uint32 * 4)()
    rc = _lib.load().gft_debug_scan_plan(tb.ctypes.data, to.ctypes.data, len(terms), lds_max, forced.encode(), C.byref(kernel), plan)
    if rc:
        raise Refused(rc, "")
    return kernel.value.decode(), dict(zip(("max_term_len", "s5_term_bits", "s5_pos_bias", "fifo_cap"), list(plan)))


def learned_unit(kernel, fifo_cap, total, lo, hi):
    """the unit size `learn` (csrc/batch_verdict.cpp) derives from a batch of `total` matches over the text [lo, hi), on a fresh
    dictionary"""
    from gofindthem_amd import _lib
    um, dens = C.c_uint32(8192), C.c_double(0.06)
    assert _lib.load().gft_debug_learn(kernel.encode(), fifo_cap, 0, total, lo, hi, C.byref(um), C.byref(dens)) == 0
    return um.value
