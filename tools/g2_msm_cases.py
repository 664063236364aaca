"""Inputs and expected values of the G2 MSM's tests on repeated, opposite and cancelling points (tests/test_g2_msm_cases_cpu.py,
tests/test_gpu_18_g2_msm_degenerate.py).  Every base is c_i * G2 with a known logarithm c_i, so the expected result of an instance is ONE
product, (sum_{i not masked} s_i c_i mod r) * G2 by the independent Python law of tools/bn254_g2_py.py, or None for the identity.  The
points come from the model of tools/fixed_base_g2_cases.py (seeded logarithms) or, for long sequences, from g2.chain_points (logarithms
a + i d); nothing here touches the code under test.

Every builder returns (bases n x 32 words in the requested form, scalars n x 8 words, inf mask or None, expected affine point or None).
Shapes: tiled, opposite, scalar_opposite, endo_triple, one_base_ramp, with_mask over any of them, and the seeded net of net_case.
The bookkeeping (unsigned_bucket_sizes, expected_lists: which list of the combine kernel a bucket of a given size reaches under a forced piece
length), the scalars and the index logic of an instance are shared with the G1 module: tools/msm_cases_common.py."""
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import bn254_g2_py as g2  # noqa: E402
import fixed_base_g2_cases as fb2  # noqa: E402
import msm_cases_common as common  # noqa: E402
from g2_pointwise_mul_cases import point_array  # noqa: E402
# (shared with tools/g1_msm_cases.py: the scalars, the bucket sizes of a plain plan and the piece rule)
from msm_cases_common import (LONG_SEG, LONG_SPAN, SPREAD_BITS, expected_lists, scalar_words, seeded_scalars, spread_scalars,  # noqa: E402,F401
                              unsigned_bucket_sizes)

P, R = g2.P, g2.R
FORM_STD, FORM_MONT = 0, 1
GEN = g2.G2_GEN
# beta^2 of gpu-acceleration_amd/csrc/msm_kernels_g2.hpp (BETA2_STD): phi2(x, y) = (beta^2 x, y) = lambda * (x, y) on G2
BETA2 = 0x59E26BCEA0D48BACD4F263F1ACDB5C4F5763473177FFFFFE
CHAIN_FROM = 65  # sequences of this many distinct bases or more come from g2.chain_points
_LAMBDA = []


def lam():
    """the scalar of phi2 on G2: the one of the two nontrivial cube roots of unity mod r (g2.glv_lambda_beta()'s lambda and its square) with
    lambda * G2 = phi2(G2) by the independent law; found once"""
    if not _LAMBDA:
        l1 = g2.glv_lambda_beta()[0]
        _LAMBDA.extend(l for l in (l1, l1 * l1 % R) if g2.mul(GEN, l) == phi2(GEN))
        assert len(_LAMBDA) == 1
    return _LAMBDA[0]


def phi2(pt):
    return None if pt is None else (g2.smul2(pt[0], BETA2), pt[1])


def decode(bases, form):
    """the affine points of n x 32 emitted words (an all-zero record: None)"""
    ri = pow(g2.R256, -1, P)
    out = []
    for row in np.asarray(bases):
        v = [g2.words_int(row[8 * k:8 * k + 8]) for k in range(4)]
        if form == FORM_MONT:
            v = [x * ri % P for x in v]
        out.append(None if not any(v) else ((v[0], v[1]), (v[2], v[3])))
    return out


class Instance(common.Instance):
    """common.Instance over G2: the points are affine pairs of Fq2 pairs, the expected value one product by the independent law"""

    def point_words(self, form):
        return point_array(self.upts, form)

    def product(self, total):
        return g2.mul(GEN, total)


def base_points(L, seed):
    """(logarithms, points) of L distinct bases: seeded logarithms below CHAIN_FROM points, an arithmetic progression a + i d from there"""
    rnd = random.Random(seed)
    if L < CHAIN_FROM:
        logs = []
        while len(logs) < L:
            c = rnd.randrange(1, R)
            if c not in logs and R - c not in logs:
                logs.append(c)
        return logs, fb2.points(logs)
    a, d = rnd.randrange(1, R), rnd.randrange(1, 1 << 64)
    return [(a + i * d) % R for i in range(L)], g2.chain_points(a, d, L)


# ---- the shapes: raw_*() return an Instance, the functions of the same name without the prefix emit it -------------------------------------
def raw_tiled(L, T, seed, scalars=None):
    """L distinct pairs (c_j * G2, s_j) repeated T times: pair j at rows t * L + j.  Every bucket that holds a point holds T copies of it."""
    logs, pts = base_points(L, seed)
    sc = list(scalars) if scalars is not None else seeded_scalars(seed, L)
    assert len(sc) == L
    idx = np.tile(np.arange(L), T)
    return Instance(logs, pts, idx, sc, idx)


def raw_opposite(L, T, seed, extra=0, scalars=None):
    """(P_j, s_j) T + extra times and (-P_j, s_j) T times.  extra = 0: every bucket sums to the identity, and so does the instance; extra = 1: every
    bucket passes through the identity and ends at P_j.  Rows: T blocks of [P_0 .. P_{L-1}, -P_0 .. -P_{L-1}], then the extra blocks of P."""
    logs, pts = base_points(L, seed)
    sc = list(scalars) if scalars is not None else seeded_scalars(seed, L)
    assert len(sc) == L
    ulogs = logs + [R - c for c in logs]
    upts = pts + [g2.neg(p) for p in pts]
    pidx = np.concatenate([np.tile(np.arange(2 * L), T), np.tile(np.arange(L), extra)])
    return Instance(ulogs, upts, pidx, sc, pidx % L)


def raw_scalar_opposite(L, seed):
    """(P_j, s_j) and (P_j, r - s_j): nothing cancels inside a bucket (the digits differ), the total is the identity"""
    logs, pts = base_points(L, seed)
    sc = seeded_scalars(seed, L)
    idx = np.arange(L)
    return Instance(logs, pts, np.concatenate([idx, idx]), sc + [R - s for s in sc], np.concatenate([idx, L + idx]))


def raw_endo_triple(L, seed, distinct=False):
    """bases P_j, phi2(P_j), phi2^2(P_j) (logarithms c, lambda c, lambda^2 c).  distinct = False: the three carry the same scalar s_j and sum to
    the identity (1 + lambda + lambda^2 = 0 mod r); True: three scalars of their own, an ordinary point.  Under the GLV split the record
    phi2(P_j) the kernel makes for the base P_j and the caller's own base phi2(P_j) are the same point in two records."""
    logs, pts = base_points(L, seed)
    l1 = lam()
    ulogs = logs + [c * l1 % R for c in logs] + [c * l1 * l1 % R for c in logs]
    p1 = [phi2(p) for p in pts]
    upts = pts + p1 + [phi2(p) for p in p1]
    sc = seeded_scalars(seed, 3 * L if distinct else L)
    pidx = np.arange(3 * L)
    return Instance(ulogs, upts, pidx, sc, pidx if distinct else pidx % L)


RAMP_LOG = 0x2F0C5A7E11D3B9A86C4E20197F5D3B1A0C9E8D7F6A5B4C3D2E1F0A9B8C7D6E5  # the logarithm of one_base_ramp's base


def raw_one_base_ramp(m, c, sign="same", log=RAMP_LOG):
    """the ONE base P = log * G2, m times, with the scalars 1, 2, ..., m < 2^c.  With c-bit plain digits and no GLV split, bucket b of the lowest
    window holds exactly P and every other window is empty: every pair level and every bit sum adds equal points.  sign = "alt": the base
    of row j is (-1)^j P, adjacent buckets are opposite.  Expected: (sum +-(j + 1)) * log * G2."""
    assert 0 < m < (1 << c) and sign in ("same", "alt")
    pt = fb2.points([log])[0]
    pidx = np.arange(m) % 2 if sign == "alt" else np.zeros(m, np.int64)
    return Instance([log, R - log], [pt, g2.neg(pt)], pidx, list(range(1, m + 1)), np.arange(m))


def raw_with_mask(inst, seed):
    """`inst` with about a quarter of its rows masked as infinity (every other one of them with zeroed base words, as a caller that keeps no
    coordinates for such a point would pass them) and about a sixth carrying the scalar 0; at least one row of each kind, and one row left alone"""
    inf, zeroed, uscal, sidx = common.mask_rows(inst, seed)
    return Instance(inst.ulogs, inst.upts, inst.pidx, uscal, sidx, inf, zeroed)


def tiled(L, T, seed, form=FORM_MONT, scalars=None):
    return raw_tiled(L, T, seed, scalars).emit(form)


def opposite(L, T, seed, form=FORM_MONT, extra=0, scalars=None):
    return raw_opposite(L, T, seed, extra, scalars).emit(form)


def scalar_opposite(L, seed, form=FORM_MONT):
    return raw_scalar_opposite(L, seed).emit(form)


def endo_triple(L, seed, form=FORM_MONT, distinct=False):
    return raw_endo_triple(L, seed, distinct).emit(form)


def one_base_ramp(m, c, sign="same", form=FORM_MONT):
    return raw_one_base_ramp(m, c, sign).emit(form)


def with_mask(inst, seed, form=FORM_MONT):
    return raw_with_mask(inst, seed).emit(form)


# ---- the seeded net: 40 combinations of size, bases, scalars, mask, window width, digit flags and forced piece length ------------------------
NET_SEED, NET_CASES, NET_CHAIN = 20261019, 40, 4096
NET_A, NET_D = 0x6F3B2A1908F7E6D5C4B3A29180F7E6D5C4B3A291, 0x9E3779B97F4A7C15
FLAG_UNSIGNED_DIGITS, FLAG_NO_GLV = common.FLAG_UNSIGNED_DIGITS, common.FLAG_NO_GLV  # MSM_FLAG_* of include/msm_hip.h
BASE_MODES = ("distinct", "odd rows = row 0", "every third negated", "all equal")
SCALAR_MODES = ("uniform", "all equal", "three distinct", "below 2^32", "60 % zeros", "all r - 1")
_CHAIN = []


def net_chain():
    if not _CHAIN:
        _CHAIN.append(g2.chain_points(NET_A, NET_D, NET_CHAIN))
    return _CHAIN[0]


def net_case(it, n=None):
    """(combination, Instance) number `it` of the net; n overrides the drawn size (the CPU test checks every mode at a small one).  The
    combination is a dict of everything that was drawn: a failing case reports it whole."""
    rng = np.random.default_rng([NET_SEED, it])
    drawn = int(rng.choice([rng.integers(1, 41), rng.integers(40, 801), rng.integers(800, 3001)]))
    n = drawn if n is None else n
    off = int(rng.integers(0, NET_CHAIN - n + 1))
    bmode, smode = it % len(BASE_MODES), int(rng.integers(0, len(SCALAR_MODES)))
    chain = net_chain()
    logs = [(NET_A + (off + i) * NET_D) % R for i in range(n)]
    pts = chain[off:off + n]
    if bmode == 1:
        for i in range(1, n, 2):
            logs[i], pts[i] = logs[0], pts[0]
    elif bmode == 2:
        for i in range(2, n, 3):
            logs[i], pts[i] = R - logs[i], g2.neg(pts[i])
    elif bmode == 3:
        logs, pts = [logs[0]] * n, [pts[0]] * n
    rnd = random.Random(int(rng.integers(0, 1 << 62)))
    sc = [rnd.randrange(R) for _ in range(n)]
    if smode == 1:
        sc = [sc[0]] * n
    elif smode == 2:
        sc = [sc[i % 3] for i in range(n)]
    elif smode == 3:
        sc = [s & 0xFFFFFFFF for s in sc]
    elif smode == 4:
        sc = [0 if rnd.random() < 0.6 else s for s in sc]
    elif smode == 5:
        sc = [R - 1] * n
    density = [None, 0.001, 0.05, 0.9][int(rng.integers(0, 4))]
    inf = None if density is None else (rng.random(n) < density).astype(np.uint8)
    combo = dict(case=it, n=n, offset=off, bases=BASE_MODES[bmode], scalars=SCALAR_MODES[smode], inf_density=density,
                 window_bits=int(rng.choice([0, 5, 8, 11, 13])), flags=int(rng.choice([0, FLAG_NO_GLV, FLAG_UNSIGNED_DIGITS, FLAG_NO_GLV | FLAG_UNSIGNED_DIGITS])),
                 piece_len=[None, "1", "2", "7"][int(rng.integers(0, 4))])
    idx = np.arange(n)
    return combo, Instance(logs, pts, idx, sc, idx, inf)
