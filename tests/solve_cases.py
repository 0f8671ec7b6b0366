"""The solver's plan and kernel variants for the tests (test infrastructure): gft_debug_plan_solve and the compiled shape of
a program set as Python values, and the small families of test_gpu_solve_variants.py -- a dictionary of three dozen terms,
programs of all three interpreter classes and of 1 .. 9 and more chunks, without rare words, with NOT / narrow INORD words,
and with one wide INORD group on top."""
import ctypes as C
import functools

import numpy as np

import inord_trees as T

# An MI355X as the engine sees it: LDS per workgroup, CUs.  Plans made with these constants are the engine's own only on such a
# device (the engine plans with its device's lds_max and its CUs less the margin it leaves); for the small sets of this module
# the choices of kernel hold for any lds_max from 64 KiB up and any number of CUs -- only `grid` follows the CUs.
LDS_MAX, N_CUS = 160 * 1024, 256
PLAN_FIELDS = ("group_docs", "p_in_lds", "prog_in_lds", "rare", "dbg_variant", "tile_words", "wide_cap", "lds_bytes", "per_cu",
               "grid", "has_kernel")


def plan_solve(n_slots, n_exprs, fprog_words, has_rare, wide_pairs, lds_max, n_cus, n_docs, forced_group=-1, prog_lds=1, dbg=0):
    from gofindthem_amd import _lib
    out = (C.c_uint64 * len(PLAN_FIELDS))()
    rc = _lib.load().gft_debug_plan_solve(n_slots, n_exprs, fprog_words, has_rare, wide_pairs, lds_max, n_cus, n_docs, forced_group,
                                          prog_lds, dbg, C.addressof(out))
    assert rc == 0, rc
    return dict(zip(PLAN_FIELDS, (int(x) for x in out)))


def compiled_shape(progs, n_slots):
    """what plan_solve reads of the set as gft_set_programs compiles it, and the interpreter class of every block of 64"""
    from gofindthem_amd import _lib
    words = np.asarray([w for p in progs for w in p], dtype=np.uint32)
    off = np.zeros(len(progs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in progs])
    shape = np.zeros(3 + max(1, (len(progs) + 63) // 64), np.uint32)
    rc = _lib.load().gft_debug_program_shape(words.ctypes.data, off.ctypes.data, len(progs), n_slots, shape.ctypes.data, len(shape))
    assert rc == 0, rc
    return {"fprog_words": int(shape[0]), "has_rare": int(shape[1]), "wide_pairs": int(shape[2]), "blk_class": shape[3:].tolist()}


# ---- the families of test_gpu_solve_variants.py -------------------------------------------------------------------------
FLAT_LEAVES = (1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 16, 17, 20, 29, 32, 33, 36)     # a fused word per leaf: 1, 2, 3, 4, 5, 8 and 9 chunks
CHUNKS = {1, 2, 3, 4, 5, 8, 9}


def _leaf(rng, terms):
    return ("not " if rng.integers(4) == 0 else "") + T.q(terms[int(rng.integers(len(terms)))])


def _flat(rng, terms, n):
    """n leaves joined without parentheses: no push, no pop"""
    e = _leaf(rng, terms)
    for _ in range(n - 1):
        e += (" and " if rng.integers(2) else " or ") + _leaf(rng, terms)
    return e


def _both(rng, terms, depth):
    """both operands of every operator are subtrees of the same depth: the accumulator stack gets `depth` deep"""
    if depth == 0:
        return "(%s %s %s)" % (_leaf(rng, terms), "and" if rng.integers(2) else "or", _leaf(rng, terms))
    e = "(%s %s %s)" % (_both(rng, terms, depth - 1), "and" if rng.integers(2) else "or", _both(rng, terms, depth - 1))
    return "not " + e if rng.integers(5) == 0 else e


def stack_depths(fam):
    """accumulator-stack depth of every fused program of a family without INORD groups (gft_debug_eval_programs' out_depth)"""
    from gofindthem_amd import _lib
    progs, n_slots = fam.programs(), len(fam.terms) + 1
    words = np.asarray([w for p in progs for w in p], dtype=np.uint32)
    off = np.zeros(len(progs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in progs])
    hit, p8, depth = np.zeros(len(progs), np.uint8), np.zeros(n_slots, np.uint8), np.zeros(len(progs), np.uint32)
    rc = _lib.load().gft_debug_eval_programs(words.ctypes.data, off.ctypes.data, len(progs), n_slots, p8.ctypes.data, hit.ctypes.data,
                                             depth.ctypes.data)
    assert rc == 0, rc
    return depth


def one_program(fam, i):
    """(chunks, interpreter class) of expression i compiled on its own"""
    s = compiled_shape([fam.programs()[i]], len(fam.terms) + 1)
    return s["fprog_words"] // 4, s["blk_class"][0]


@functools.lru_cache(maxsize=None)
def family(rare):
    """rare 0: 64 programs of every interpreter class -- flat ones of FLAT_LEAVES leaves, trees nested 1-2 deep (two registers)
    and 3-7 deep (four registers, beyond them scratch) --; 1: NOT over groups and narrow INORD groups on top; 2: and one wide
    INORD group.  130 documents that hold 4 to 32 of the 36 terms each."""
    rng = np.random.default_rng(4100)
    terms = T._pool(36, rng)
    exprs = [_flat(rng, terms, FLAT_LEAVES[i % len(FLAT_LEAVES)]) for i in range(64)]
    exprs += [_both(rng, terms, 1 + i % 2) for i in range(64)]
    exprs += [_both(rng, terms, (3, 4, 3, 4, 5, 3, 4, 6, 5, 3, 4, 7, 3, 4, 5, 6)[i % 16]) for i in range(64)]
    if rare >= 1:
        while len(exprs) < 192 + 24:
            e = T.gen_expr(rng, terms, lambda: int(rng.integers(2, 7)), p_or=0.4, max_groups=2)
            if T.classify(T.words_of(e)) == T.NARROW:
                exprs.append(e)
        exprs += ["not (inord(%s and %s))" % (T.q(terms[0]), T.q(terms[1])), "%s and %s" % (_both(rng, terms, 5), T.gen_group(rng, terms, 4, 0.3))]
    if rare >= 2:
        qa, qb = [T.q(t) for t in terms[:18]], [T.q(t) for t in terms[18:]]
        # (twice 35 leaves: 70 pairs alive; terms repeat)
        exprs.append("inord(%s and %s)" % (T.flat(qa + qa[:17], "or"), T.flat(qb + qb[:17], "or")))
        assert T.classify(T.words_of(exprs[-1])) == T.WIDE
    exprs = [exprs[int(i)] for i in rng.permutation(len(exprs))]
    texts = [T._subset_doc(rng, terms, int(rng.integers(4, 33))) for _ in range(130)]
    return T.Family("variants-rare%d" % rare, terms, exprs, texts)
