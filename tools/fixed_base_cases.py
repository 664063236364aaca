"""Inputs and expected values of the G1 fixed-base multiplication's tests (tests/test_fixed_base_cpu.py, tests/test_gpu_11_fixed_base.py) and of
tools/fixed_base_timing.py: the edge scalars of a window width, seeded 256-bit patterns, and k * P from the CPU oracle with k reduced modulo r in
Python -- nothing here touches the code under test."""
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
GEN = (1, 2)
MONT_R = (1 << 256) % R  # arkworks Fr.0 holds k * MONT_R mod r


def words(v):
    return orc.int_to_words(v)


def to_words(vs):
    return np.stack([words(v) for v in vs]) if len(vs) else np.zeros((0, 8), np.uint32)


def num_windows(c):
    return -(-257 // c)


def edge_scalars(c):
    """the scalars every window width must get right: the multiples of r (k * P is the identity), r - 1 (= -P), the ends of the 256-bit range,
    2^(c j) - 1 (all digits below window j at their largest: a chain of carries) and 2^(c j - 1) (the one digit that stays +2^(c-1)) for every
    window, and the word whose every digit is 2^(c-1)"""
    ks = [0, 1, 2, R - 1, R, R + 1, 2 * R, 5 * R, 1 << 255, (1 << 256) - 1]
    for j in range(1, num_windows(c)):
        if c * j <= 256:
            ks += [(1 << (c * j)) - 1, 1 << (c * j - 1)]
    ks.append(sum(1 << (c * j + c - 1) for j in range(num_windows(c)) if c * j + c - 1 < 256))
    return ks


def patterns(seed, n):
    """n seeded 256-bit patterns (about five in six are >= r)"""
    rnd = random.Random(seed)
    return [rnd.getrandbits(256) for _ in range(n)]


def base_words(xy, form=FORM_STD):
    x, y = xy
    if form == FORM_MONT:
        x, y = x * (1 << 256) % P, y * (1 << 256) % P
    return np.concatenate([words(x), words(y)])


def point(k, base=GEN):
    """(k mod r) * base as (x, y) integers, None for the identity"""
    xy, inf = orc.g1_to_affine_std(orc.g1_scalar_mul(base_words(base), words(k % R)))
    return None if inf else (orc.words_to_int(xy[:8]), orc.words_to_int(xy[8:]))


def expected(ks, base=GEN, out_std=False):
    """(n x 16 words, n bytes) the call must give for the integers ks: canonical coordinates in the output form, zeros and inf = 1 for the identity"""
    ks = [k % R for k in ks]
    xy, inf = np.zeros((len(ks), 16), np.uint32), np.zeros(len(ks), np.uint8)
    live = [i for i, k in enumerate(ks) if k]
    for i, k in enumerate(ks):
        inf[i] = 0 if k else 1
    if not live:
        return xy, inf
    if base == GEN:
        xy[live] = orc.gen_bases_from_logs(to_words([ks[i] for i in live]), FORM_STD if out_std else FORM_MONT)
    else:
        for i in live:
            xy[i] = base_words(point(ks[i], base), FORM_STD if out_std else FORM_MONT)
    return xy, inf
