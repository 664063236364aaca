"""The BN254 G1 group law on the device, one operation at a time (-m gpu), on RAW limb records: xyzz_madd (normalised and raw-negated y),
xyzz_madd_m32, xyzz_add, xyzz_dbl of csrc/ec_bn254.hpp and the eight-lane addition of csrc/ec_wide.hpp (records in LDS, in place, and in global
memory) through msm_test_g1_raw_op, which hands the kernel the limbs the test wrote and returns the limbs it stored.  msm_test_g1_op
(tests/test_gpu_1_parity.py) converts canonical words on the way in and reduces on the way out, so it only ever shows the law operands below 1.1p
and hides the representative of the result; here the test chooses the representative -- reduced (LOW), or at the top of the documented ranges
(TOP: X + 6p, Y + 4p, ZZ + p, ZZZ + p; affine y as y, y + p and 2p - y; any 256-bit words for the M256 path) -- and checks every element of every
launch with tools/g1_ops_cases.check_output: every limb <= 2^29 - 1, X < 7p, Y < 5p, ZZ, ZZZ < 2p, ZZ^3 == ZZZ^2, the affine point bit-exactly
the Python sum (tools/bn254_py.py), identity results with ZZ zero limb for limb.  Integer work: no tolerance anywhere.
tools/fp_bounds_check.cpp (tests/test_fp_bounds.py) runs the same operand classes through the host compile of the scalar functions with every
limb assumption asserted: that is the check that these inputs are legal."""
import os
import random
import sys

import numpy as np
import pytest

import mopro_msm_hip as mh
from mopro_msm_hip import testhooks as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import g1_ops_cases as gc  # noqa: E402

pytestmark = pytest.mark.gpu
bn, P, R, G = gc.bn, gc.P, gc.R_ORDER, gc.G
MADD, MADD_NEG_RAW, M256, M256_NEG = th.OP_G1_RAW_MADD, th.OP_G1_RAW_MADD_NEG_RAW, th.OP_G1_RAW_MADD_M256, th.OP_G1_RAW_MADD_M256_NEG
ADD, DBL, WIDE_LDS, WIDE_HBM = th.OP_G1_RAW_ADD, th.OP_G1_RAW_DBL, th.OP_G1_RAW_ADD_WIDE_LDS, th.OP_G1_RAW_ADD_WIDE_HBM
ADDS = (("add", ADD), ("wide lds", WIDE_LDS), ("wide hbm", WIDE_HBM))
NP = 65
INFL = {"low": gc.LOW, "top": gc.TOP}
ONE = gc.enc(1)
check_all = gc.check_all


def arr(rows):
    return np.array(rows, np.uint32)


def ids(ident, m):
    return arr([ident] * m)


# ---- shared operands and references, made once -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    c = th.HooksContext()
    yield c
    c.close()


@pytest.fixture(scope="module")
def data():
    rnd = random.Random(0x61)
    pts = gc.chain_points(2 * NP)          # 130 points: P_i = (A0 + i D0) G, Q_i = (A0 + (NP + i) D0) G
    ps, qs = pts[:NP], pts[NP:]
    d = {"rnd": rnd, "P": ps, "Q": qs, "kP": [gc.A0 + i * gc.D0 for i in range(NP)], "kQ": [gc.A0 + (NP + i) * gc.D0 for i in range(NP)]}
    d["tp"], d["tq"] = [rnd.randrange(1, P) for _ in ps], [rnd.randrange(1, P) for _ in qs]
    for name, infl in INFL.items():
        d["P_" + name] = arr([gc.record(p_, t, infl) for p_, t in zip(ps, d["tp"])])
        d["Q_" + name] = arr([gc.record(q_, t, infl) for q_, t in zip(qs, d["tq"])])
    for s in gc.SPELLINGS:
        d["q_" + s] = arr([gc.affine_record(q_, s) for q_ in qs])
    d["q_words"] = arr([gc.words_m256(q_) for q_ in qs])
    d["q_words_nc"] = arr([gc.words_m256(q_, True) for q_ in qs])
    # arbitrary 256-bit words (off the curve: pair_of_words), every fifth element all ones
    d["any_words"] = arr([gc.ALL_ONES_WORDS if i % 5 == 0 else [rnd.getrandbits(32) for _ in range(16)] for i in range(NP)])
    d["any_pairs"] = [gc.pair_of_words(w) for w in d["any_words"]]
    d["P+Q"] = [bn.add(p_, q_) for p_, q_ in zip(ps, qs)]
    d["P-Q"] = [bn.add(p_, bn.neg(q_)) for p_, q_ in zip(ps, qs)]
    d["2P"] = [bn.add(p_, p_) for p_ in ps]
    d["P+any"] = [bn.add(p_, w) for p_, w in zip(ps, d["any_pairs"])]
    d["P-any"] = [bn.add(p_, bn.neg(w)) for p_, w in zip(ps, d["any_pairs"])]
    assert all(bn.is_on_curve(p_) for p_ in ps[:3] + qs[-3:]) and qs[-1] == bn.mul(d["kQ"][-1], G)
    return d


# ---- 1. element counts and operand mixes: the scalar functions ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_scalar_ops_reduced_inflated_and_mixed(ctx, data, n):
    d, op = data, ctx.test_g1_raw_op
    for a in ("low", "top"):
        acc = d["P_" + a][:n]
        for s, want in (("canonical", "P+Q"), ("plus_p", "P+Q"), ("negated", "P-Q")):
            check_all(op(MADD, acc, d["q_" + s][:n]), d[want][:n], "madd %s, y %s" % (a, s))
        check_all(op(MADD_NEG_RAW, acc, d["q_canonical"][:n]), d["P-Q"][:n], "madd %s, y negated raw in the kernel" % a)
        for words, plus, minus in (("q_words", "P+Q", "P-Q"), ("q_words_nc", "P+Q", "P-Q"), ("any_words", "P+any", "P-any")):
            check_all(op(M256, acc, d[words][:n]), d[plus][:n], "madd_m32 %s, %s" % (a, words))
            check_all(op(M256_NEG, acc, d[words][:n]), d[minus][:n], "madd_m32 negated %s, %s" % (a, words))
        for b in ("low", "top"):
            check_all(op(ADD, acc, d["Q_" + b][:n]), d["P+Q"][:n], "add %s %s" % (a, b))
        check_all(op(DBL, acc), d["2P"][:n], "dbl " + a)


# ---- 2. the eight-lane addition: partial groups of a wavefront, a partial last workgroup ------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 8, 9, 65])
def test_wide_ops_reduced_inflated_and_mixed(ctx, data, n):
    d, op = data, ctx.test_g1_raw_op
    for a in ("low", "top"):
        for b in ("low", "top"):
            pa, qb = d["P_" + a][:n], d["Q_" + b][:n]
            scalar = op(ADD, pa, qb)
            check_all(scalar, d["P+Q"][:n], "add %s %s" % (a, b))
            for name, w in ADDS[1:]:
                out = op(w, pa, qb)
                check_all(out, d["P+Q"][:n], "%s %s %s" % (name, a, b))
                assert [gc.to_affine(r) for r in out] == [gc.to_affine(r) for r in scalar]  # point for point the scalar addition's result


# ---- 3. special cases, reduced and inflated, through every operation that can reach them -------------------------------------------------------
M = 5  # elements per special-case launch


@pytest.mark.parametrize("infl", ["low", "top"])
def test_identity_operands_in_both_encodings(ctx, data, infl):
    d, op = data, ctx.test_g1_raw_op
    recs = d["P_" + infl][:M]
    for idname, ident in (("one", gc.ID_ONE), ("zero", gc.ID_ZERO)):
        idm = ids(ident, M)
        for name, w in ADDS:
            out = op(w, idm, recs)          # identity + P: P comes back limb for limb
            assert (out == recs).all(), (name, idname)
            check_all(out, d["P"][:M], name + ": id + P")
            out = op(w, recs, idm)
            assert (out == recs).all(), (name, idname)
            check_all(out, d["P"][:M], name + ": P + id")
            for ident2 in (gc.ID_ONE, gc.ID_ZERO):
                check_all(op(w, idm, ids(ident2, M)), [None] * M, name + ": id + id")
        check_all(op(DBL, idm), [None] * M, "2 id")
        # identity accumulator of the mixed additions: the affine point itself with ZZ = ZZZ = 1
        for s in gc.SPELLINGS:
            q = d["q_" + s][:M]
            out = op(MADD, idm, q)          # q.x, normalize(q.y), 1, 1: the operand's own limbs
            check_all(out, [gc.affine_of(r) for r in q], "id madd Q, y " + s)
            assert (out[:, :18] == q).all() and (out[:, 18:27] == arr(ONE)).all() and (out[:, 27:] == arr(ONE)).all()
        out = op(MADD_NEG_RAW, idm, d["q_canonical"][:M])  # the raw 2p - y, normalised: the limbs of the "negated" spelling
        check_all(out, [bn.neg(q_) for q_ in d["Q"][:M]], "id madd -Q (raw)")
        assert (out[:, :18] == d["q_negated"][:M]).all() and (out[:, 18:27] == arr(ONE)).all() and (out[:, 27:] == arr(ONE)).all()
        for words, pairs in (("q_words", d["Q"]), ("q_words_nc", d["Q"]), ("any_words", d["any_pairs"])):
            for w, sign in ((M256, False), (M256_NEG, True)):
                out = op(w, idm, d[words][:M])
                check_all(out, [bn.neg(q_) if sign else q_ for q_ in pairs[:M]], "id madd_m32 %s" % words)
                assert (out[:, 18:27] == arr(ONE)).all() and (out[:, 27:] == arr(ONE)).all()
                assert all(gc.value(r[9:18]) < 4 * P and gc.value(r[:9]) < 2 * P for r in out)  # X < 2p, Y < 4p: xyzz_madd_m32's identity start


@pytest.mark.parametrize("infl_b", ["low", "top"])
@pytest.mark.parametrize("infl_a", ["low", "top"])
def test_doubling_and_cancelling_through_the_additions(ctx, data, infl_a, infl_b):
    d, rnd, op = data, data["rnd"], ctx.test_g1_raw_op
    a = d["P_" + infl_a][:M]
    other_t = [t * rnd.randrange(2, P) % P for t in d["tp"][:M]]
    same = d["P_" + infl_b][:M]                                                                   # the same ZZ (the same record when infl_a == infl_b)
    rescaled = arr([gc.record(p_, t, INFL[infl_b]) for p_, t in zip(d["P"], other_t)])             # the same point under another ZZ
    negated = arr([gc.record(bn.neg(p_), t, INFL[infl_b]) for p_, t in zip(d["P"], other_t)])      # -P under another ZZ
    assert not (rescaled[:, 18:27] == a[:, 18:27]).all(axis=1).any()
    for name, w in ADDS:
        check_all(op(w, a, same), d["2P"][:M], name + ": P + P, same ZZ")
        check_all(op(w, a, rescaled), d["2P"][:M], name + ": P + P, another ZZ")
        check_all(op(w, rescaled, a), d["2P"][:M], name + ": P + P, another ZZ, swapped")
        for out in (op(w, a, negated), op(w, negated, a)):
            check_all(out, [None] * M, name + ": P + (-P)")
            assert (out == ids(gc.ID_ONE, M)).all(), name  # exactly what xyzz_identity() writes


@pytest.mark.parametrize("infl", ["low", "top"])
def test_doubling_and_cancelling_through_the_mixed_additions(ctx, data, infl):
    d, op = data, ctx.test_g1_raw_op
    ps, a = d["P"][:M], d["P_" + infl][:M]
    negs = [bn.neg(p_) for p_ in ps]
    identity = ids(gc.ID_ONE, M)
    # every spelling of y: "negated" holds the NEGATION of the pair it is built from
    same = {"canonical": ps, "plus_p": ps, "negated": negs}
    for s in gc.SPELLINGS:
        check_all(op(MADD, a, arr([gc.affine_record(p_, s) for p_ in same[s]])), d["2P"][:M], "P madd P, y " + s)
        opposite = negs if s != "negated" else ps
        out = op(MADD, a, arr([gc.affine_record(p_, s) for p_ in opposite]))
        check_all(out, [None] * M, "P madd (-P), y " + s)
        assert (out == identity).all(), s
    check_all(op(MADD_NEG_RAW, a, arr([gc.affine_record(p_) for p_ in negs])), d["2P"][:M], "P madd -(-P), raw")
    out = op(MADD_NEG_RAW, a, arr([gc.affine_record(p_) for p_ in ps]))
    check_all(out, [None] * M, "P madd -P, raw")
    assert (out == identity).all()
    for nc in (False, True):  # both signs of the M256 path, canonical and non-canonical words
        w_p, w_n = arr([gc.words_m256(p_, nc) for p_ in ps]), arr([gc.words_m256(p_, nc) for p_ in negs])
        check_all(op(M256, a, w_p), d["2P"][:M], "P madd_m32 P")
        check_all(op(M256_NEG, a, w_n), d["2P"][:M], "P madd_m32 -(-P)")
        for out in (op(M256, a, w_n), op(M256_NEG, a, w_p)):
            check_all(out, [None] * M, "P madd_m32 (-P)")
            assert (out == identity).all()


@pytest.mark.parametrize("infl", ["low", "top"])
def test_mixed_addition_of_a_y_of_exactly_2p(ctx, data, infl):
    """2p - 0 = 2p: the largest affine y a negation can hand over (normalised: the "negated" spelling; raw: fp_neg_raw<2> in the kernel).  The pairs
    (x, 0) are not on the curve (BN254 has no point of order two) and need not be: the chord is a rational function of the coordinates.  The
    tangent at such a pair does not exist, so these operands meet accumulators with another x only."""
    d, rnd, op = data, data["rnd"], ctx.test_g1_raw_op
    pairs = [(rnd.randrange(1, P), 0) for _ in range(M - 1)] + [(P - 1, 0)]
    q = arr([gc.affine_record(pr, "negated") for pr in pairs])
    assert all(gc.value(r[9:]) == 2 * P for r in q)
    q0 = arr([gc.affine_record(pr) for pr in pairs])  # the same residues, zero as zero
    a = d["P_" + infl][:M]
    want = [bn.add(p_, pr) for p_, pr in zip(d["P"], pairs)]
    out = op(MADD, a, q)
    check_all(out, want, "P madd (x, 2p)")
    ref = op(MADD, a, q0)
    check_all(ref, want, "P madd (x, 0)")
    residues = lambda recs: [[gc.residue(r[9 * k:9 * k + 9]) for k in range(4)] for r in recs]
    assert residues(out) == residues(ref)                          # the same residues in every coordinate as on the reduced operand
    raw = op(MADD_NEG_RAW, a, q0)                                  # fp_neg_raw<2>(0): the pad 2p itself, unnormalised, as the multiplier
    check_all(raw, want, "P madd (x, raw 2p)")
    assert residues(raw) == residues(ref)
    for ident in (gc.ID_ONE, gc.ID_ZERO):                          # identity accumulator: Y comes out as the normalised 2p
        for o, b in ((MADD, q), (MADD_NEG_RAW, q0)):
            out = op(o, ids(ident, M), b)
            check_all(out, pairs, "id madd (x, 2p)")
            assert (out[:, :18] == q).all()


@pytest.mark.parametrize("n", [1, 9])
def test_operands_in_the_last_sliver_below_the_bounds(ctx, data, n):
    """X = 7p - 1 - d, Y = 5p - 1 - d, affine x = p - 1 - d, y = 2p - 1 - d (d < 2^20): the largest subtrahends the header allows, so a pad that is
    too small for them goes negative whatever the minuend (tools/g1_ops_cases.near_top_record).  Every operation, the doubling and the cancelling
    branches included; the pairs are off the curve (rational functions, as the any-words pairs)"""
    d, rnd, op = data, data["rnd"], ctx.test_g1_raw_op
    near = [gc.near_top_record(rnd.randrange(1, P), rnd) for _ in range(n)]
    a, pa = arr([r for r, _ in near]), [pr for _, pr in near]
    other = [gc.near_top_record(rnd.randrange(1, P), rnd) for _ in range(n)]
    b, pb = arr([r for r, _ in other]), [pr for _, pr in other]
    aff = [gc.near_top_affine(rnd) for _ in range(n)]
    q, pq = arr([r for r, _ in aff]), [pr for _, pr in aff]
    aff_c = [gc.near_top_affine(rnd, canonical_y=True) for _ in range(n)]  # y = p - 1 - d: the top of what the kernel may negate raw
    qc, pqc = arr([r for r, _ in aff_c]), [pr for _, pr in aff_c]
    assert all(7 * P - (1 << 20) <= gc.value(r[:9]) < 7 * P and 5 * P - (1 << 20) <= gc.value(r[9:18]) < 5 * P for r in a)
    assert all(P - (1 << 20) <= gc.value(r[:9]) < P and 2 * P - (1 << 20) <= gc.value(r[9:]) < 2 * P for r in q)
    check_all(a, pa, "the builder's own records")
    add2 = lambda xs, ys: [bn.add(x, y) for x, y in zip(xs, ys)]
    negs = lambda xs: [bn.neg(x) for x in xs]
    check_all(op(MADD, a, q), add2(pa, pq), "madd near, near")
    check_all(op(MADD_NEG_RAW, a, qc), add2(pa, negs(pqc)), "madd near, raw negation of y near p")
    check_all(op(M256, a, d["any_words"][:n]), add2(pa, d["any_pairs"]), "madd_m32 near, any words")
    check_all(op(M256_NEG, a, d["any_words"][:n]), add2(pa, negs(d["any_pairs"])), "madd_m32 negated near, any words")
    check_all(op(DBL, a), add2(pa, pa), "dbl near")
    for name, w in ADDS:
        check_all(op(w, a, b), add2(pa, pb), name + ": near + near")
        check_all(op(w, a, d["Q_top"][:n]), add2(pa, d["Q"]), name + ": near + top")
        check_all(op(w, d["Q_low"][:n], a), add2(pa, d["Q"]), name + ": low + near")
        check_all(op(w, a, a), add2(pa, pa), name + ": near + itself")
        # the same pair, and its negation, under another ZZ
        same = arr([gc.record(pr, rnd.randrange(1, P), gc.TOP) for pr in pa])
        opposite = arr([gc.record(bn.neg(pr), rnd.randrange(1, P), gc.TOP) for pr in pa])
        check_all(op(w, a, same), add2(pa, pa), name + ": near + the same pair")
        check_all(op(w, same, a), add2(pa, pa), name + ": the same pair + near")
        for out in (op(w, a, opposite), op(w, opposite, a)):
            check_all(out, [None] * n, name + ": near + its negation")
            assert (out == ids(gc.ID_ONE, n)).all()
    # the mixed additions' own special branches: the accumulator holds the near-top affine pair, or its negation
    for o, b, pb_, sign in ((MADD, q, pq, 1), (MADD_NEG_RAW, qc, pqc, -1)):
        added = pb_ if sign > 0 else negs(pb_)  # the pair the operation adds
        acc_same = arr([gc.record(pr, rnd.randrange(1, P), gc.TOP) for pr in added])
        acc_opposite = arr([gc.record(bn.neg(pr), rnd.randrange(1, P), gc.TOP) for pr in added])
        check_all(op(o, acc_same, b), add2(added, added), "doubling branch, y at the top of its range")
        out = op(o, acc_opposite, b)
        check_all(out, [None] * n, "cancelling branch, y at the top of its range")
        assert (out == ids(gc.ID_ONE, n)).all()


# ---- 4. special pairs next to ordinary ones in one wavefront: the vote / fallback path and the eight-lane path in one launch ------------------
@pytest.mark.parametrize("infl", ["low", "top"])
def test_wide_special_pairs_beside_ordinary_pairs(ctx, data, infl):
    d, rnd, op = data, data["rnd"], ctx.test_g1_raw_op
    top = INFL[infl]
    n = 19  # two full 64-lane workgroups of eight pairs and a partial one
    a, b, want = [], [], []
    kinds = ("plain", "id+P", "plain", "P+P", "P+id", "plain", "P-P", "id+id", "P+P'", "plain")
    for i in range(n):
        kind = kinds[i % len(kinds)]
        p_, q_, rec, qrec = d["P"][i], d["Q"][i], list(d["P_" + infl][i]), list(d["Q_" + infl][i])
        ident = gc.ID_ONE if i % 2 else gc.ID_ZERO
        t2 = d["tp"][i] * rnd.randrange(2, P) % P
        row = {"plain": (rec, qrec, d["P+Q"][i]), "id+P": (ident, rec, p_), "P+id": (rec, ident, p_), "id+id": (ident, gc.ID_ONE, None),
               "P+P": (rec, rec, d["2P"][i]), "P+P'": (gc.record(p_, t2, top), rec, d["2P"][i]),
               "P-P": (rec, gc.record(bn.neg(p_), t2, top), None)}[kind]
        a.append(row[0]), b.append(row[1]), want.append(row[2])
    assert {kinds[i % len(kinds)] for i in range(8)} >= {"plain", "id+P", "P+P", "P+id", "P-P", "id+id"}  # all in the first wavefront
    a, b = arr(a), arr(b)
    scalar = op(ADD, a, b)
    check_all(scalar, want, "add")
    for name, w in ADDS[1:]:
        out = op(w, a, b)
        check_all(out, want, name)
        assert [gc.to_affine(r) for r in out] == [gc.to_affine(r) for r in scalar]
        special = [i for i in range(n) if kinds[i % len(kinds)] != "plain"]
        assert (out[special] == scalar[special]).all()  # the fallback IS the scalar addition: the same limbs


# ---- 5. chains: the records fed back are the device's own outputs ------------------------------------------------------------------------------
def test_chain_of_64_doublings_then_added_to_itself(ctx, data):
    d, op = data, ctx.test_g1_raw_op
    n = 3
    cur = np.concatenate([d["P_top"][:n], d["P_low"][:n]])
    ks = d["kP"][:n] * 2
    want = d["P"][:n] * 2
    for step in range(64):
        cur = op(DBL, cur)
        want = [bn.add(p_, p_) for p_ in want]
        check_all(cur, want, "dbl chain step %d" % step)
    assert want == [bn.mul(k << 64, G) for k in ks]
    want = [bn.mul(k << 65, G) for k in ks]
    for name, w in ADDS:
        check_all(op(w, cur, cur), want, name + ": 2^64 P + 2^64 P")


@pytest.mark.parametrize("path", ["limbs", "m256"])
def test_fold_of_64_affine_points_with_alternating_signs(ctx, data, path):
    d, op = data, ctx.test_g1_raw_op
    lanes = 4  # lane j folds Q_j, Q_(j+1), ... with a sign pattern shifted per lane pair; the accumulators start as both identity encodings
    acc = arr([gc.ID_ONE, gc.ID_ZERO, gc.ID_ZERO, gc.ID_ONE])
    sums, want = [0] * lanes, [None] * lanes
    for step in range(64):
        ng = step % 2 == 1  # one launch per step: the sign is the operation's (MADD / MADD_NEG_RAW, M256 / M256_NEG); lanes differ in the point
        idx = [(step + 7 * j) % NP for j in range(lanes)]
        if path == "limbs":
            b = d["q_plus_p" if step % 3 == 2 and not ng else "q_canonical"][idx]
            acc = op(MADD_NEG_RAW if ng else MADD, acc, b)
        else:
            b = d["q_words_nc" if step % 3 == 2 else "q_words"][idx]
            acc = op(M256_NEG if ng else M256, acc, b)
        for j, i in enumerate(idx):
            q_ = bn.neg(d["Q"][i]) if ng else d["Q"][i]
            want[j] = bn.add(want[j], q_)
            sums[j] += -d["kQ"][i] if ng else d["kQ"][i]
        check_all(acc, want, "fold step %d" % step)
    assert want == [bn.mul(s % R, G) for s in sums]


def test_pairwise_tree_of_64_records_in_six_wide_launches(ctx, data):
    d, op = data, ctx.test_g1_raw_op
    cur = np.concatenate([d["P_top"][:32], d["Q_low"][:32]])
    want = d["P"][:32] + d["Q"][:32]
    launches = 0
    while len(cur) > 1:
        h = len(cur) // 2
        cur = op(WIDE_LDS, cur[:h], cur[h:])
        want = [bn.add(x, y) for x, y in zip(want[:h], want[h:])]
        check_all(cur, want, "tree level of %d" % h)
        launches += 1
    assert launches == 6 and want == [bn.mul((sum(d["kP"][:32]) + sum(d["kQ"][:32])) % R, G)]


# ---- 6. the hook's own argument checks ---------------------------------------------------------------------------------------------------------
def test_hook_refuses_malformed_input(ctx, data):
    lib, h = ctx._lib, ctx._h
    a, b, q, w = data["P_low"][:2].copy(), data["Q_low"][:2].copy(), data["q_canonical"][:2].copy(), data["any_words"][:2].copy()
    out = np.zeros_like(a)
    call = lambda op, a_, b_, n: lib.msm_test_g1_raw_op(h, op, mh._p32(a_), mh._p32(b_), mh._p32(out), n)
    assert all(call(op, a, b, 2) == mh.OK for op in (ADD, WIDE_LDS, WIDE_HBM)) and call(DBL, a, None, 2) == mh.OK
    assert call(MADD, a, q, 2) == mh.OK and call(MADD_NEG_RAW, a, q, 2) == mh.OK
    assert int(w.max()) == 0xFFFFFFFF and call(M256, a, w, 2) == mh.OK and call(M256_NEG, a, w, 2) == mh.OK  # 16-word b: any 32-bit values
    assert call(ADD, a, b, 0) == mh.ERR_EMPTY
    assert all(call(op, a, None, 2) == mh.ERR_BAD_ARG for op in range(8) if op != DBL)
    assert call(8, a, b, 2) == mh.ERR_BAD_ARG and call(0xFFFFFFFF, a, b, 2) == mh.ERR_BAD_ARG
    assert lib.msm_test_g1_raw_op(h, ADD, None, mh._p32(b), mh._p32(out), 2) == mh.ERR_BAD_ARG
    assert lib.msm_test_g1_raw_op(h, ADD, mh._p32(a), mh._p32(b), None, 2) == mh.ERR_BAD_ARG
    out[:] = 0
    for word in (0, 8, 35 + 36):  # a limb of 2^29 or more, anywhere in a or b (the top limb included), is refused before anything runs
        bad = a.copy()
        bad.reshape(-1)[word] = 1 << 29
        assert all(call(op, bad, b, 2) == mh.ERR_BAD_ARG and call(op, a, bad, 2) == mh.ERR_BAD_ARG for op in (ADD, WIDE_LDS, WIDE_HBM))
        assert call(DBL, bad, None, 2) == mh.ERR_BAD_ARG and call(MADD, bad, q, 2) == mh.ERR_BAD_ARG and call(M256, bad, w, 2) == mh.ERR_BAD_ARG
    for word in (0, 17, 18 + 17):
        badq = q.copy()
        badq.reshape(-1)[word] = 0xFFFFFFFF
        assert call(MADD, a, badq, 2) == mh.ERR_BAD_ARG and call(MADD_NEG_RAW, a, badq, 2) == mh.ERR_BAD_ARG
    assert not out.any()  # nothing was written by any refused call
    with pytest.raises(mh.MsmError) as e:
        ctx.test_g1_raw_op(ADD, bad, b)
    assert e.value.code == mh.ERR_BAD_ARG
    check_all(ctx.test_g1_raw_op(ADD, a, b), data["P+Q"][:2], "the context still works")
