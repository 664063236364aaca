"""Inputs and expected values of the G2 element-wise multiplication's tests (tests/test_g2_pointwise_mul_cpu.py,
tests/test_gpu_17_g2_pointwise_mul.py) and of tools/g2_pointwise_mul_timing.py: bases Q_i = b_i * H and the products (k_i * b_i mod r) * H from
the model of tools/fixed_base_g2_cases.py, which is built on the independent Python law of tools/bn254_g2_py.py; the edge scalars, the seeded
patterns, the logarithms and the split are those of the G1 tests (tools/pointwise_mul_cases.py, imported as they are); the three-entry table in
Python integers over Fq2 -- nothing here touches the code under test."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import bn254_g2_py as g2  # noqa: E402
import fixed_base_g2_cases as fb2  # noqa: E402
import pointwise_mul_cases as pm  # noqa: E402

P, R = g2.P, g2.R
assert (P, R) == (pm.P, pm.R)
FORM_STD, FORM_MONT = 0, 1
MONT_R = pm.MONT_R
LAMBDA, BETA, HALF_BITS = pm.LAMBDA, pm.BETA, pm.HALF_BITS
BETA2 = BETA * BETA % P  # phi2(x, y) = (beta^2 x, y) = lambda * (x, y) on G2
edge_scalars, patterns, logs, split, to_words, words = pm.edge_scalars, pm.patterns, pm.logs, pm.split, pm.to_words, pm.words
GEN = g2.G2_GEN


def phi2(pt):
    return (g2.smul2(pt[0], BETA2), pt[1])


def table(pt, k):
    """P1 = sign(k1) * Q, P2 = sign(k2) * lambda * Q = (beta^2 x, +-y), S = P1 + P2 for the canonical k, by the independent law"""
    k1, k2 = split(k % R)
    p1 = g2.neg(pt) if k1 < 0 else pt
    p2 = phi2(pt)
    p2 = g2.neg(p2) if k2 < 0 else p2
    return p1, p2, g2.add(p1, p2)


def base_points(bs):
    """[b_i * H] as affine points (b_i != 0 mod r)"""
    return fb2.points([b % R for b in bs])


def bases(bs, form=FORM_MONT):
    """Q_i = b_i * H as n x 32 words"""
    return point_array(base_points(bs), form)


def point_array(pts, form=FORM_MONT):
    """n x 32 words of affine points; None becomes a zero record"""
    xy = np.zeros((len(pts), 32), np.uint32)
    for i, pt in enumerate(pts):
        if pt is not None:
            xy[i] = g2.point_words(pt, form == FORM_MONT)
    return xy


def expected(ks, bs, inf=None, out_std=False):
    """(n x 32 words, n bytes) the call must give for the scalars ks (integers, as the call reads them: reduced here) on the bases b_i * H:
    (k_i * b_i mod r) * H, zeros and inf = 1 where the product is 0 mod r or the base is flagged"""
    prod = [0 if (inf is not None and inf[i]) else (ks[i] % R) * (bs[i] % R) % R for i in range(len(ks))]
    return fb2.expected(prod, GEN, out_std)


def expected_points(ks, pts, out_std=False):
    """the same for arbitrary points of G2 (None: flagged), one g2.mul each"""
    out = [None if pt is None else g2.mul(pt, k % R) for k, pt in zip(ks, pts)]
    return point_array(out, FORM_STD if out_std else FORM_MONT), np.array([1 if o is None else 0 for o in out], np.uint8)


def point_ints(rec_std):
    """the four integers of a record of 32 words"""
    return tuple(g2.words_int(rec_std[8 * c:8 * c + 8]) for c in range(4))
