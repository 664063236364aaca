"""CPU side of the raw-limb G1 group-law hook (msm_test_g1_raw_op) and of the net tests/test_gpu_20_g1_ops.py casts with it: the symbol lives in
the hooks build only, the header's op numbers are the Python constants, a NULL context is refused, the wrapper checks shapes before it calls, and
the operand builders / check_output of tools/g1_ops_cases.py accept what they must and REJECT every kind of wrong record they exist to catch.  No
production code is mutated: the last part tests the checker on records built wrong on purpose."""
import os
import re
import sys

import numpy as np
import pytest

import mopro_msm_hip as mh
from mopro_msm_hip import testhooks as th
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import g1_ops_cases as gc  # noqa: E402

P = gc.P
RAW_OPS = ("MADD", "MADD_NEG_RAW", "MADD_M256", "MADD_M256_NEG", "ADD", "DBL", "ADD_WIDE_LDS", "ADD_WIDE_HBM")


def test_raw_hook_lives_in_the_hooks_build_only():
    assert "msm_test_g1_raw_op" in th.HOOK_SYMBOLS
    assert hasattr(th.load_hooks_library(), "msm_test_g1_raw_op") and not hasattr(mh.load_library(), "msm_test_g1_raw_op")
    assert "msm_test_g1_raw_op" not in open(os.path.join(ROOT, "include", "msm_hip.h")).read()


def test_header_defines_match_the_python_constants():
    hdr = open(os.path.join(ROOT, "include", "msm_hip_testhooks.h")).read()
    found = dict(re.findall(r"#define MSM_OP_G1_RAW_(\w+) (\d+)u\b", hdr))
    assert sorted(found) == sorted(RAW_OPS)
    for name in RAW_OPS:
        assert int(found[name]) == getattr(th, "OP_G1_RAW_" + name), name
    assert sorted(th.G1_RAW_B_WORDS) == list(range(8))
    assert [th.G1_RAW_B_WORDS[getattr(th, "OP_G1_RAW_" + name)] for name in RAW_OPS] == [18, 18, 16, 16, 36, 0, 36, 36]


def test_raw_hook_refuses_a_null_context():
    lib = th.load_hooks_library()
    a, b, out = np.zeros((1, 36), np.uint32), np.zeros((1, 36), np.uint32), np.zeros((1, 36), np.uint32)
    for op in range(8):
        assert lib.msm_test_g1_raw_op(None, op, mh._p32(a), mh._p32(b), mh._p32(out), 1) == mh.ERR_BAD_ARG
    assert not out.any()


def test_raw_wrapper_checks_shapes_before_the_call():
    """a missing or shorter b would let the C hook read past the buffer: the wrapper raises before it calls (no context is touched)"""
    call = th.HooksContext.test_g1_raw_op
    a = np.zeros((3, 36), np.uint32)
    for op in range(8):
        if op != th.OP_G1_RAW_DBL:
            with pytest.raises(ValueError):
                call(None, op, a, None)
            with pytest.raises(ValueError):
                call(None, op, a, np.zeros((2, th.G1_RAW_B_WORDS[op]), np.uint32))  # one record short
    with pytest.raises(ValueError):
        call(None, th.OP_G1_RAW_MADD, a, np.zeros((3, 16), np.uint32))   # 48 words: not a whole number of 18-limb records
    with pytest.raises(ValueError):
        call(None, th.OP_G1_RAW_MADD_M256, a, np.zeros((3, 18), np.uint32))
    with pytest.raises(ValueError):
        call(None, 8, a, a)
    with pytest.raises(ValueError):
        call(None, th.OP_G1_RAW_DBL, np.zeros(35, np.uint32))  # not a whole record


# ---- the builders and the checker ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pts():
    p = gc.chain_points(3)
    assert all(gc.bn.is_on_curve(q) for q in p) and p[1] == gc.bn.mul(gc.A0 + gc.D0, gc.G)
    return p


def test_builders_round_trip(pts):
    pt, t = pts[0], 0x1D2C3B4A5968778695A4B3C2D1E0F
    low, top = gc.record(pt, t, gc.LOW), gc.record(pt, t, gc.TOP)
    gc.check_output(low, pt, "low")
    gc.check_output(top, pt, "top")
    for k in range(4):  # the same residues, TOP exactly TOP[k] * p above LOW: inside the header's range, in its last p
        lo, hi = gc.value(low[9 * k:9 * k + 9]), gc.value(top[9 * k:9 * k + 9])
        assert lo < P and hi == lo + gc.TOP[k] * P and (gc.BOUNDS[k] - 1) * P <= hi < gc.BOUNDS[k] * P
    assert gc.value(gc.enc(5, 6)) == 5 * gc.R261 % P + 6 * P and gc.residue(gc.enc(7, 3)) == 7
    # the three spellings of an affine y
    assert gc.affine_of(gc.affine_record(pt)) == pt and gc.affine_of(gc.affine_record(pt, "plus_p")) == pt
    assert gc.affine_of(gc.affine_record(pt, "negated")) == gc.bn.neg(pt)
    y = lambda s, q=pt: gc.value(gc.affine_record(q, s)[9:])
    assert y("canonical") < P <= y("plus_p") == y("canonical") + P < 2 * P and y("negated") == 2 * P - y("canonical")
    assert y("negated", (5, 0)) == 2 * P                                          # 2p - 0: exactly 2p
    assert max(gc.affine_record((5, 0), "negated")) <= gc.MASK
    # arkworks words, canonical and + p, and what any 16 words stand for
    w, wn = gc.words_m256(pt), gc.words_m256(pt, True)
    assert gc.pair_of_words(w) == pt == gc.pair_of_words(wn) and w != wn and max(wn) <= 0xFFFFFFFF
    assert gc.bn.from_words(wn[:8]) == gc.bn.from_words(w[:8]) + P
    ones = gc.pair_of_words(gc.ALL_ONES_WORDS)
    assert ones[0] == ones[1] == (gc.R256 - 1) * gc.R256_INV % P
    # records and affine operands in the last sliver below the bounds hold the pair they report
    import random
    rnd = random.Random(7)
    rec, pair = gc.near_top_record(t, rnd)
    gc.check_output(rec, pair, "near top")
    assert 7 * P - (1 << 20) <= gc.value(rec[:9]) < 7 * P and 5 * P - (1 << 20) <= gc.value(rec[9:18]) < 5 * P
    aff, apair = gc.near_top_affine(rnd)
    assert gc.affine_of(aff) == apair and P - (1 << 20) <= gc.value(aff[:9]) < P and 2 * P - (1 << 20) <= gc.value(aff[9:]) < 2 * P
    aff, apair = gc.near_top_affine(rnd, canonical_y=True)
    assert gc.affine_of(aff) == apair and P - (1 << 20) <= gc.value(aff[9:]) < P
    # both identity encodings are identities for the checker
    gc.check_output(gc.ID_ONE, None)
    gc.check_output(gc.ID_ZERO, None)
    assert gc.to_affine(gc.ID_ONE) is None and gc.to_affine(low) == pt == gc.to_affine(top)


def _with(rec, k, limbs9):
    r = list(rec)
    r[9 * k:9 * k + 9] = limbs9
    return r


def test_check_output_rejects_what_it_exists_to_catch(pts):
    pt, other, t = pts[0], pts[1], 0xABCDEF0123456789ABCDEF
    good = gc.record(pt, t, gc.TOP)
    gc.check_output(good, pt)
    rejected = {}
    # one limb set to 2^29 (value kept: the limb below takes the carry back): an output that is not normalised
    for word in (0, 9 + 3, 18 + 7, 27 + 0):
        bad, c = list(good), word - word % 9
        bad[word] += 1 << 29
        bad[word + 1] -= 1
        assert bad[word + 1] >= 0 and gc.value(bad[c:c + 9]) == gc.value(good[c:c + 9])
        rejected["limb %d" % word] = bad
    x, y, zz, zzz = (gc.residue(c) for c in gc.coords(good))
    rejected["X at 7p"] = _with(good, 0, gc.limbs(x * gc.R261 % P + 7 * P))
    rejected["Y at 5p"] = _with(good, 1, gc.limbs(y * gc.R261 % P + 5 * P))
    rejected["ZZ at 2p"] = _with(good, 2, gc.limbs(zz * gc.R261 % P + 2 * P))
    rejected["ZZZ at 2p"] = _with(good, 3, gc.limbs(zzz * gc.R261 % P + 2 * P))
    rejected["wrong point"] = gc.record(other, t, gc.TOP)
    rejected["negated point"] = gc.record(gc.bn.neg(pt), t, gc.TOP)
    rejected["ZZ^3 != ZZZ^2"] = _with(_with(good, 1, gc.enc(y * 2 % P)), 3, gc.enc(zzz * 2 % P))  # Y / ZZZ is still the point's y
    rejected["identity for a point"] = gc.ID_ONE
    rejected["ZZ a multiple of p"] = _with(good, 2, gc.limbs(P))
    for what, bad in rejected.items():
        with pytest.raises(AssertionError):
            gc.check_output(bad, pt, what)
    assert gc.to_affine(rejected["ZZ^3 != ZZZ^2"]) == pt  # only the consistency check can have refused that one
    # the bounds are exact: Y = 5p - 1 passes (as the point it then is), Y = 5p does not
    y_top = (5 * P - 1) * gc.R261_INV % P
    gc.check_output(_with(good, 1, gc.limbs(5 * P - 1)), (pt[0], y_top * pow(zzz, -1, P) % P))
    with pytest.raises(AssertionError):
        gc.check_output(_with(good, 1, gc.limbs(5 * P)), (pt[0], 0))
    # an "identity" whose ZZ has a non-zero limb (p is zero modulo p, not zero limb for limb), and a point where the identity is due
    with pytest.raises(AssertionError):
        gc.check_output(_with(gc.ID_ONE, 2, gc.limbs(P)), None)
    with pytest.raises(AssertionError):
        gc.check_output(_with(gc.ID_ZERO, 2, [0] * 8 + [1]), None)
    with pytest.raises(AssertionError):
        gc.check_output(good, None)
    # the bounds hold for identity results as well
    with pytest.raises(AssertionError):
        gc.check_output(_with(gc.ID_ONE, 0, gc.limbs(7 * P)), None)
    with pytest.raises(AssertionError):
        gc.check_all([good], [pt, pt])
