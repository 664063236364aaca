"""Inputs and expected values of the G1 element-wise multiplication's tests (tests/test_pointwise_mul_cpu.py, tests/test_gpu_14_pointwise_mul.py)
and of tools/pointwise_mul_timing.py: bases P_i = b_i * G and the products (k_i * b_i mod r) * G from the CPU oracle, the edge scalars of the
GLV split and the joint ladder, seeded 256-bit patterns, and the split and the three-entry table in Python integers from
tests/golden/glv_constants.json -- nothing here touches the code under test."""
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import bn254_oracle as orc  # noqa: E402

P, R = orc.P, orc.R_ORDER
FORM_STD, FORM_MONT = 0, 1
MONT_R = (1 << 256) % R  # arkworks Fr.0 holds k * MONT_R mod r
_G = json.load(open(os.path.join(ROOT, "tests", "golden", "glv_constants.json")))
LAMBDA, BETA = int(_G["lambda"], 16), int(_G["beta"], 16)
HALF_BITS = int(_G["half_bits"])


def words(v):
    return orc.int_to_words(v)


def to_words(vs, width=8):
    return np.stack([orc.int_to_words(v, width) for v in vs]) if len(vs) else np.zeros((0, width), np.uint32)


def patterns(seed, n):
    """n seeded 256-bit patterns (about five in six are >= r)"""
    rnd = random.Random(seed)
    return [rnd.getrandbits(256) for _ in range(n)]


def split(k):
    """(k1, k2) signed, k = k1 + lambda * k2 (mod r), of the canonical k < r: the rounded quotients of tools/gen_glv_constants.py"""
    a1, b1, a2, b2 = (int(_G[t]) for t in ("a1", "b1", "a2", "b2"))
    sh = int(_G["quotient_shift"])
    c1 = (k * int(_G["g1"], 16) + (1 << (sh - 1))) >> sh  # round(k * |b2| / r)
    d2 = (k * int(_G["g2"], 16) + (1 << (sh - 1))) >> sh  # round(k * |b1| / r)
    k1, k2 = k - c1 * a1 + d2 * a2, d2 * b2 - c1 * b1
    assert (k1 + LAMBDA * k2 - k) % R == 0
    return k1, k2


def big_half_scalars(seed, count):
    """seeded scalars below r whose split has a half of at least 2^125: the top position of the ladder is in use"""
    rnd, out = random.Random(seed), []
    while len(out) < count:
        k = rnd.getrandbits(256) % R
        if max(abs(h) for h in split(k)) >= 1 << (HALF_BITS - 1):
            out.append(k)
    return out


def edge_scalars():
    """what the reduction, the split and the ladder must get right: the multiples of r and their neighbours, the ends of the 256-bit range,
    lambda and its neighbours, scalars with a half of zero (small k: k2 = 0; small multiples of lambda: k1 = 0), equal and opposite halves
    (the ladder starts on S or uses nothing else), single bits and runs of ones, and halves that reach the top position"""
    ks = [0, 1, 2, 3, R - 1, R, R + 1, 2 * R, 5 * R, 1 << 255, (1 << 256) - 1]
    ks += [LAMBDA, LAMBDA + 1, LAMBDA - 1, R - LAMBDA, LAMBDA * LAMBDA % R]
    ks += [m * LAMBDA % R for m in (2, 3, 5, 0xFFFF)] + [4, 7, 0xFFFF, (1 << 64) + 1]
    ks += [m * (1 + LAMBDA) % R for m in (1, 2, 3, 0x1234567)] + [m * (1 - LAMBDA) % R for m in (1, 2, 3, 0x1234567)]
    for j in range(0, 254, 7):
        ks += [1 << j, (1 << j) - 1]
    return ks + big_half_scalars(0x9A1F, 6)


def neg(pt):
    return (pt[0], (P - pt[1]) % P)


def add(a, b):
    """a + b for two affine points with different x"""
    l = (b[1] - a[1]) * pow(b[0] - a[0], -1, P) % P
    x = (l * l - a[0] - b[0]) % P
    return x, (l * (a[0] - x) - a[1]) % P


def table(pt, k):
    """P1 = sign(k1) * P, P2 = sign(k2) * lambda * P = (beta x, +-y), S = P1 + P2 for the canonical k"""
    k1, k2 = split(k % R)
    p1 = neg(pt) if k1 < 0 else pt
    p2 = (BETA * pt[0] % P, pt[1])
    p2 = neg(p2) if k2 < 0 else p2
    return p1, p2, add(p1, p2)


def logs(seed, n):
    """n seeded nonzero logarithms b_i of the bases"""
    rnd = random.Random(seed)
    return [rnd.randrange(1, R) for _ in range(n)]


def bases(bs, form=FORM_MONT):
    """P_i = b_i * G as n x 16 words (b_i != 0 mod r)"""
    return orc.gen_bases_from_logs(to_words([b % R for b in bs]), form)


def expected(ks, bs, inf=None, out_std=False):
    """(n x 16 words, n bytes) the call must give for the scalars ks (integers, as the call reads them: reduced here) on the bases b_i * G:
    (k_i * b_i mod r) * G, zeros and inf = 1 where the product is 0 mod r or the base is flagged"""
    n = len(ks)
    prod = [0 if (inf is not None and inf[i]) else (ks[i] % R) * (bs[i] % R) % R for i in range(n)]
    xy, out_inf = np.zeros((n, 16), np.uint32), np.array([0 if v else 1 for v in prod], np.uint8)
    live = [i for i, v in enumerate(prod) if v]
    if live:
        xy[live] = orc.gen_bases_from_logs(to_words([prod[i] for i in live]), FORM_STD if out_std else FORM_MONT)
    return xy, out_inf


def point_ints(rec_std):
    return orc.words_to_int(rec_std[:8]), orc.words_to_int(rec_std[8:])
