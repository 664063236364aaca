"""The BN254 G2 group law on the device, one operation at a time (-m gpu): xyzz2_madd / xyzz2_add / xyzz2_dbl of csrc/ec_g2_bn254.hpp through
msm_test_g2_op, which hands the kernel RAW limb records and returns the limbs it stored.  The test chooses the representative the device computes
on -- reduced, or at the top of the documented ranges (X + 11p, Y + 7p, ZZ + 3p, ZZZ + 3p; affine y as y and as 2p - y) -- and checks every
output: the affine point is bit-exactly the Python sum (tools/bn254_g2_py.py), ZZ^3 == ZZZ^2, every limb <= 2^29 - 1, every component below the
header's bounds (X < 12p, Y < 8p, ZZ, ZZZ < 4.2p), identity results have ZZ exactly zero.  tools/g2_bounds_check.cpp (tests/test_g2_bounds.py)
runs the same operand classes on the host with every limb assumption asserted: that is the check that these inputs are legal."""
import os
import random
import sys

import numpy as np
import pytest

import mopro_msm_hip as mh
from mopro_msm_hip import testhooks as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bn254_g2_py as g2  # noqa: E402

pytestmark = pytest.mark.gpu
P, R, G = g2.P, g2.R, g2.G2_GEN
R261 = 1 << 261
R261_INV = pow(R261, -1, P)
MASK = (1 << 29) - 1
MADD, ADD, DBL = th.OP_G2_MADD, th.OP_G2_ADD, th.OP_G2_DBL
A0, D0 = 0x1234567890ABCDEF1234567890ABCDEF, 0xFEDCBA987654321  # P_i = (A0 + i * D0) * G2
NP = 65
TOP = (11, 7, 3, 3)   # multiples of p added to X, Y, ZZ, ZZZ: the top of the documented ranges
LOW = (0, 0, 0, 0)


# ---- records -----------------------------------------------------------------------------------------------------------------------------------
def limbs(v):
    assert 0 <= v < R261
    return [(v >> (29 * i)) & MASK for i in range(9)]


def enc(v, k=0):
    """9 x 29-bit limbs of v * 2^261 mod p + k * p"""
    return limbs(v * R261 % P + k * P)


def value(ws):
    return sum(int(w) << (29 * i) for i, w in enumerate(ws))


def residue(ws):
    return value(ws) * R261_INV % P


def enc2(a, k=0):
    return enc(a[0], k) + enc(a[1], k)


def record(pt, t, infl=LOW):
    """the XYZZ record (x t^2, y t^3, t^2, t^3) of an affine pair, each coordinate on the representative + infl[.] * p"""
    t2 = g2.mul2(t, t)
    t3 = g2.mul2(t2, t)
    return enc2(g2.mul2(pt[0], t2), infl[0]) + enc2(g2.mul2(pt[1], t3), infl[1]) + enc2(t2, infl[2]) + enc2(t3, infl[3])


def affine_record(pt, negate=False):
    """x canonical; y canonical, or 2p - y per component as k_g2_accumulate's fp2_neg<2> gives it (2p exactly for a zero component): the point -pt"""
    y = [enc(c) for c in pt[1]]
    if negate:
        y = [limbs(2 * P - value(c)) for c in y]
    return enc2(pt[0]) + y[0] + y[1]


ID_ONE = enc2((1, 0)) + enc2((1, 0)) + [0] * 36  # what xyzz2_identity() writes
ID_ZERO = [0] * 72                               # what k_g2_clear_empty writes


def arr(rows):
    return np.array(rows, np.uint32)


def fq2_of(rec, k):
    return (residue(rec[18 * k:18 * k + 9]), residue(rec[18 * k + 9:18 * k + 18]))


def is_identity(rec):
    return not np.asarray(rec[36:54]).any()


def to_affine(rec):
    """record -> affine pair (X / ZZ, Y / ZZZ), None for the identity"""
    if is_identity(rec):
        return None
    return (g2.mul2(fq2_of(rec, 0), g2.inv2(fq2_of(rec, 2))), g2.mul2(fq2_of(rec, 1), g2.inv2(fq2_of(rec, 3))))


def check_output(rec, want, what=""):
    """every property the header promises of an output record, and the point itself"""
    rec = [int(w) for w in rec]
    assert max(rec) <= MASK, what
    for k, (num, den) in enumerate(((12, 1), (8, 1), (21, 5), (21, 5))):  # X < 12p, Y < 8p, ZZ < 4.2p, ZZZ < 4.2p
        for c in range(2):
            v = value(rec[18 * k + 9 * c:18 * k + 9 * c + 9])
            assert den * v < num * P, (what, ("X", "Y", "ZZ", "ZZZ")[k], v / P)
    if want is None:
        assert is_identity(rec), what  # ZZ exactly zero, limb for limb
        return
    assert not is_identity(rec), what
    zz, zzz = fq2_of(rec, 2), fq2_of(rec, 3)
    assert g2.mul2(g2.mul2(zz, zz), zz) == g2.mul2(zzz, zzz), what
    assert to_affine(rec) == want, what


def check_all(out, wants, what=""):
    assert len(out) == len(wants)
    for i, (rec, want) in enumerate(zip(out, wants)):
        check_output(rec, want, (what, i))


# ---- shared operands and references, made once -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    c = th.HooksContext()
    yield c
    c.close()


@pytest.fixture(scope="module")
def data():
    rnd = random.Random(0x62)
    rand2 = lambda: (rnd.randrange(1, P), rnd.randrange(P))
    pts = g2.chain_points(A0, D0, 2 * NP, block=2 * NP)
    ps, qs = pts[:NP], pts[NP:]
    d = {"rnd": rnd, "rand2": rand2, "P": ps, "Q": qs}
    d["tp"], d["tq"] = [rand2() for _ in ps], [rand2() for _ in qs]
    for name, infl in (("low", LOW), ("top", TOP)):
        d["P_" + name] = arr([record(p_, t, infl) for p_, t in zip(ps, d["tp"])])
        d["Q_" + name] = arr([record(q_, t, infl) for q_, t in zip(qs, d["tq"])])
    d["q_aff"] = arr([affine_record(q_) for q_ in qs])
    d["q_aff_neg"] = arr([affine_record(q_, negate=True) for q_ in qs])
    d["P+Q"] = [g2.add(p_, q_) for p_, q_ in zip(ps, qs)]
    d["P-Q"] = [g2.add(p_, g2.neg(q_)) for p_, q_ in zip(ps, qs)]
    d["2P"] = [g2.add(p_, p_) for p_ in ps]
    assert all(g2.on_curve(p_) for p_ in ps[:3] + qs[:3])
    return d


def test_helpers_round_trip(data):
    """the test's own records: a reduced and an inflated record hold the same point, within the preconditions"""
    for name in ("low", "top"):
        for rec, p_ in list(zip(data["P_" + name], data["P"]))[:4]:
            check_output(rec, p_, name)
    assert value(enc(5, 11)) == 5 * R261 % P + 11 * P and residue(enc(7, 3)) == 7
    assert residue(affine_record(data["Q"][0], True)[18:27]) == (-data["Q"][0][1][0]) % P
    assert value(affine_record(((1, 2), (0, 5)), True)[18:27]) == 2 * P  # a zero component negated: exactly 2p


# ---- 1. element counts and operand mixes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_every_op_reduced_inflated_and_mixed(ctx, data, n):
    d = data
    check_all(ctx.test_g2_op(MADD, d["P_low"][:n], d["q_aff"][:n]), d["P+Q"][:n], "madd low, y")
    check_all(ctx.test_g2_op(MADD, d["P_top"][:n], d["q_aff_neg"][:n]), d["P-Q"][:n], "madd top, 2p - y")
    check_all(ctx.test_g2_op(MADD, d["P_top"][:n], d["q_aff"][:n]), d["P+Q"][:n], "madd top, y")
    check_all(ctx.test_g2_op(MADD, d["P_low"][:n], d["q_aff_neg"][:n]), d["P-Q"][:n], "madd low, 2p - y")
    for a in ("low", "top"):
        for b in ("low", "top"):
            check_all(ctx.test_g2_op(ADD, d["P_" + a][:n], d["Q_" + b][:n]), d["P+Q"][:n], "add %s %s" % (a, b))
        check_all(ctx.test_g2_op(DBL, d["P_" + a][:n]), d["2P"][:n], "dbl " + a)


# ---- 2. special cases, reduced and inflated ----------------------------------------------------------------------------------------------------
M = 5  # elements per special-case launch


@pytest.mark.parametrize("infl", ["low", "top"])
def test_identity_operands_in_both_encodings(ctx, data, infl):
    d = data
    recs = d["P_" + infl][:M]
    for name, ident in (("one", ID_ONE), ("zero", ID_ZERO)):
        ids = arr([ident] * M)
        out = ctx.test_g2_op(ADD, ids, recs)       # identity + P: P comes back limb for limb
        assert (out == recs).all(), name
        check_all(out, d["P"][:M], "id + P")
        out = ctx.test_g2_op(ADD, recs, ids)
        assert (out == recs).all(), name
        check_all(out, d["P"][:M], "P + id")
        for name2, ident2 in (("one", ID_ONE), ("zero", ID_ZERO)):
            check_all(ctx.test_g2_op(ADD, ids, arr([ident2] * M)), [None] * M, "id + id")
        check_all(ctx.test_g2_op(DBL, ids), [None] * M, "2 id")
        # identity accumulator of the mixed addition: the affine point itself with ZZ = ZZZ = 1
        for q, want in ((d["q_aff"], d["Q"]), (d["q_aff_neg"], [g2.neg(q_) for q_ in d["Q"]])):
            out = ctx.test_g2_op(MADD, ids, q[:M])
            check_all(out, want[:M], "id madd Q")
            assert (out[:, :36] == q[:M]).all() and (out[:, 36:54] == arr(enc2((1, 0)))).all() and (out[:, 54:] == arr(enc2((1, 0)))).all()


@pytest.mark.parametrize("infl_b", ["low", "top"])
@pytest.mark.parametrize("infl_a", ["low", "top"])
def test_doubling_and_cancelling_through_the_addition(ctx, data, infl_a, infl_b):
    d = data
    top = {"low": LOW, "top": TOP}
    a = d["P_" + infl_a][:M]
    other_t = [g2.mul2(t, d["rand2"]()) for t in d["tp"][:M]]
    same = d["P_" + infl_b][:M]                                                             # the same ZZ (the same record when infl_a == infl_b)
    rescaled = arr([record(p_, t, top[infl_b]) for p_, t in zip(d["P"], other_t)])          # the same point under another ZZ
    negated = arr([record(g2.neg(p_), t, top[infl_b]) for p_, t in zip(d["P"], other_t)])   # -P under another ZZ
    assert not (rescaled[:, 36:] == a[:, 36:]).all()
    check_all(ctx.test_g2_op(ADD, a, same), d["2P"][:M], "P + P, same t")
    check_all(ctx.test_g2_op(ADD, a, rescaled), d["2P"][:M], "P + P, another t")
    check_all(ctx.test_g2_op(ADD, rescaled, a), d["2P"][:M], "P + P, another t, swapped")
    for out in (ctx.test_g2_op(ADD, a, negated), ctx.test_g2_op(ADD, negated, a)):
        check_all(out, [None] * M, "P + (-P)")
        assert (out == arr([ID_ONE] * M)).all()  # exactly what xyzz2_identity() writes


@pytest.mark.parametrize("infl", ["low", "top"])
def test_doubling_and_cancelling_through_the_mixed_addition(ctx, data, infl):
    d = data
    a = d["P_" + infl][:M]
    p_aff = arr([affine_record(p_) for p_ in d["P"][:M]])
    p_as_neg_of_neg = arr([affine_record(g2.neg(p_), negate=True) for p_ in d["P"][:M]])  # P given as (x, 2p - (p - y))
    p_neg = arr([affine_record(p_, negate=True) for p_ in d["P"][:M]])                      # -P given as (x, 2p - y)
    p_neg_canonical = arr([affine_record(g2.neg(p_)) for p_ in d["P"][:M]])                # -P given canonical
    check_all(ctx.test_g2_op(MADD, a, p_aff), d["2P"][:M], "P madd P")
    check_all(ctx.test_g2_op(MADD, a, p_as_neg_of_neg), d["2P"][:M], "P madd P (2p - y form)")
    for q in (p_neg, p_neg_canonical):
        out = ctx.test_g2_op(MADD, a, q)
        check_all(out, [None] * M, "P madd (-P)")
        assert (out == arr([ID_ONE] * M)).all()


@pytest.mark.parametrize("infl", ["low", "top"])
def test_mixed_addition_of_a_negated_y_with_a_zero_component(ctx, data, infl):
    """2p - 0 = 2p exactly: the largest affine operand k_g2_accumulate can hand over.  The pairs are not on the twist and need not be: the chord
    and the tangent are rational functions of the coordinates, which the Python law evaluates on any pair"""
    d, rnd = data, data["rnd"]
    top = {"low": LOW, "top": TOP}[infl]
    ys = [(0, rnd.randrange(1, P)), (rnd.randrange(1, P), 0), (0, 1), (P - 1, 0)]
    pairs = [(d["rand2"](), y) for y in ys]               # the pair whose NEGATION is added
    q = arr([affine_record(pr, negate=True) for pr in pairs])
    assert sorted(value(r[18:27]) == 2 * P for r in q) == [False, False, True, True] and sum(value(r[27:36]) == 2 * P for r in q) == 2
    q_reduced = arr([affine_record(g2.neg(pr)) for pr in pairs])  # the same residues, zero as zero
    n = len(pairs)
    a = d["P_" + infl][:n]
    want = [g2.add(p_, g2.neg(pr)) for p_, pr in zip(d["P"], pairs)]
    out = ctx.test_g2_op(MADD, a, q)
    check_all(out, want, "P madd (x, 2p - y)")
    ref = ctx.test_g2_op(MADD, a, q_reduced)              # the same operation on the reduced operand: the same residues in every component
    assert [[residue(r[9 * k:9 * k + 9]) for k in range(8)] for r in out] == [[residue(r[9 * k:9 * k + 9]) for k in range(8)] for r in ref]
    # the same pair as the accumulator: the doubling branch, entered with a y component of 2p; and the cancelling branch against +pair
    acc_same = arr([record(g2.neg(pr), d["rand2"](), top) for pr in pairs])
    check_all(ctx.test_g2_op(MADD, acc_same, q), [g2.add(g2.neg(pr), g2.neg(pr)) for pr in pairs], "doubling branch, y component 2p")
    acc_opposite = arr([record(pr, d["rand2"](), top) for pr in pairs])
    out = ctx.test_g2_op(MADD, acc_opposite, q)
    check_all(out, [None] * n, "cancelling branch, y component 2p")
    assert (out == arr([ID_ONE] * n)).all()


# ---- 3. chained use: the records fed back are the device's own outputs -------------------------------------------------------------------------
def test_chain_of_64_doublings_then_added_to_itself(ctx, data):
    d = data
    n = 3
    cur = np.concatenate([d["P_low"][:n], d["P_top"][:n]])
    ks = [(A0 + i * D0) % R for i in range(n)] * 2
    for step in range(64):
        cur = ctx.test_g2_op(DBL, cur)
        assert int(cur.max()) <= MASK
        if step % 16 == 15:
            check_all(cur, [g2.mul(G, k << (step + 1)) for k in ks], "dbl chain step %d" % step)
    check_all(cur, [g2.mul(G, k << 64) for k in ks], "2^64 P")
    check_all(ctx.test_g2_op(ADD, cur, cur), [g2.mul(G, k << 65) for k in ks], "2^64 P + 2^64 P")


def test_fold_of_64_affine_points_by_mixed_additions(ctx, data):
    d = data
    lanes = 4   # lane j folds Q_j, Q_(j+1), ... with alternating signs (lane parity shifts the pattern); accumulators start as both identities
    acc = arr([ID_ONE, ID_ZERO, ID_ONE, ID_ZERO])
    sums = [0] * lanes
    for step in range(64):
        rows = []
        for j in range(lanes):
            i, ng = (step + j) % NP, (step + j // 2) % 3 == 0
            rows.append(d["q_aff_neg"][i] if ng else d["q_aff"][i])
            k = A0 + (NP + i) * D0
            sums[j] += -k if ng else k
        acc = ctx.test_g2_op(MADD, acc, arr(rows))
        assert int(acc.max()) <= MASK
    assert all(g2.mul(G, A0 + (NP + i) * D0) == d["Q"][i] for i in (0, NP - 1))
    check_all(acc, [g2.mul(G, s % R) for s in sums], "fold of 64")
    # the same sums as one msm of the Python module over lane 0's points
    pts0, sc0 = [d["Q"][step % NP] for step in range(64)], [R - 1 if step % 3 == 0 else 1 for step in range(64)]
    assert to_affine(acc[0]) == g2.msm(pts0, sc0)


# ---- 4. the hook's own argument checks ---------------------------------------------------------------------------------------------------------
def test_hook_refuses_malformed_input(ctx, data):
    lib, h = ctx._lib, ctx._h
    a, b, q = data["P_low"][:2].copy(), data["Q_low"][:2].copy(), data["q_aff"][:2].copy()
    out = np.zeros_like(a)
    call = lambda op, a_, b_, n: lib.msm_test_g2_op(h, op, mh._p32(a_), mh._p32(b_), mh._p32(out), n)
    assert call(ADD, a, b, 2) == mh.OK and call(MADD, a, q, 2) == mh.OK and call(DBL, a, None, 2) == mh.OK
    assert call(ADD, a, b, 0) == mh.ERR_EMPTY
    assert call(ADD, a, None, 2) == mh.ERR_BAD_ARG and call(MADD, a, None, 2) == mh.ERR_BAD_ARG
    assert call(3, a, b, 2) == mh.ERR_BAD_ARG
    assert lib.msm_test_g2_op(h, ADD, None, mh._p32(b), mh._p32(out), 2) == mh.ERR_BAD_ARG
    assert lib.msm_test_g2_op(h, ADD, mh._p32(a), mh._p32(b), None, 2) == mh.ERR_BAD_ARG
    out[:] = 0
    for word in (0, 8, 71 + 72):  # a limb of 2^29 or more, anywhere in a or b (the top limb included), is refused before anything runs
        bad = a.copy()
        bad.reshape(-1)[word] = 1 << 29
        assert call(ADD, bad, b, 2) == mh.ERR_BAD_ARG and call(DBL, bad, None, 2) == mh.ERR_BAD_ARG and call(ADD, a, bad, 2) == mh.ERR_BAD_ARG
    badq = q.copy()
    badq[1, 35] = 0xFFFFFFFF
    assert call(MADD, a, badq, 2) == mh.ERR_BAD_ARG
    assert not out.any()
    with pytest.raises(mh.MsmError) as e:
        ctx.test_g2_op(ADD, bad, b)
    assert e.value.code == mh.ERR_BAD_ARG
    check_all(ctx.test_g2_op(ADD, a, b), data["P+Q"][:2], "the context still works")
