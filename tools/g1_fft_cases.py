"""Inputs and expected values of the G1 group transform's tests (tests/test_g1_fft_cpu.py, tests/test_gpu_16_g1_fft.py) and of
tools/g1_fft_timing.py: points P_j = a_j * G from seeded logarithms (the CPU oracle), the expected transform as the oracle's points of the Fr
transform of the a_j in Python integers (tools/bn254_fr_ntt_py.py), zeros as flagged identities, the structured vectors whose butterflies meet
A = T, A = -T and the identity, and the halo2 KZG parameter sets of tests/golden/srs_kzg_points.json -- nothing here touches the code under test."""
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from oracle import bn254_oracle as orc  # noqa: E402
import bn254_fr_ntt_py as frpy  # noqa: E402

P, R = orc.P, orc.R_ORDER
assert R == frpy.R
FORM_STD, FORM_MONT = 0, 1
INVERSE, OUT_STD, IN_STD = 1, 8, 16  # MSM_NTT_INVERSE, MSM_FB_OUT_STD, MSM_PM_BASES_STD
FLAG_MATRIX = [d | i | o for d in (0, INVERSE) for i in (0, IN_STD) for o in (0, OUT_STD)]
GARBAGE = 0xDEADBEEF  # the words of a flagged place in these inputs: the call must not read a point out of them


def root(log_n):
    return frpy.root(log_n)


def logs(seed, n, zero_every=0):
    """n seeded logarithms a_j; every zero_every-th (from the second) is 0: an identity among the inputs"""
    rnd = random.Random(seed)
    a = [rnd.randrange(1, R) for _ in range(n)]
    if zero_every:
        for j in range(1, n, zero_every):
            a[j] = 0
    return a


def points(a, form=FORM_MONT, fill=GARBAGE):
    """(n x 16 words, n bytes) of the points a_j * G: a_j = 0 (mod r) is flagged, its words are `fill`"""
    a = [v % R for v in a]
    xy, inf = np.full((len(a), 16), fill, np.uint32), np.array([0 if v else 1 for v in a], np.uint8)
    live = [j for j, v in enumerate(a) if v]
    if live:
        xy[live] = orc.gen_bases_from_logs(np.stack([orc.int_to_words(a[j]) for j in live]), form)
    return xy, inf


def transform_logs(a, log_n, inverse=False, batch=1):
    """the Fr transform of every array of 2^log_n logarithms, in Python integers"""
    n = 1 << log_n
    assert len(a) == n * batch
    out = []
    for b in range(batch):
        out += frpy.ntt(a[b * n:(b + 1) * n], 1, inverse)
    return out


def expected(a, log_n, flags=0, batch=1):
    """(points x 16 words, bytes) the call must leave for the inputs a_j * G: the points of the transformed logarithms in the requested form,
    sixteen zero words and inf = 1 where the logarithm is 0"""
    return points(transform_logs(a, log_n, bool(flags & INVERSE), batch), FORM_STD if flags & OUT_STD else FORM_MONT, fill=0)


def inputs(a, flags=0):
    return points(a, FORM_STD if flags & IN_STD else FORM_MONT)


def identity_cases(log_n, seed=0x1DE7):
    """name -> logarithms of the structured inputs of 2^log_n points: a constant vector (n * P at index 0, the identity elsewhere: the first
    stage meets A = T in every butterfly -- and, on the way back, A = -T); unit vectors at m in {0, 1, n/2, n-1} (outputs w^(mi) * P, every other
    input flagged); everything flagged; alternating P, -P (the first stage cancels everywhere)"""
    n = 1 << log_n
    a = random.Random(seed + log_n).randrange(1, R)
    cases = {"constant": [a] * n, "all_flagged": [0] * n, "alternating": [a if j % 2 == 0 else R - a for j in range(n)]}
    for m in sorted({0, 1, n // 2, n - 1}):
        cases["unit_%d" % m] = [a if j == m else 0 for j in range(n)]
    return cases


def edge_twiddles():
    """twiddles a single butterfly must get right: 1 and -1, the fourth root of unity and its inverse, the cube root lambda (its split has the
    half k1 = 0), 2^126 - 1 and a small one (k2 = 0), 0 (w * B is the identity: A + 0, A - 0), and a pattern above r"""
    lam = int(json.load(open(os.path.join(ROOT, "tests", "golden", "glv_constants.json")))["lambda"], 16)
    return [1, R - 1, root(2), R - root(2), lam, 3, 0, R, (1 << 256) - 1, root(10), pow(root(28), 12345, R)]


def butterfly_expected(a, b, w, out_std=False):
    """(A + w B, A - w B) for A = a * G, B = b * G (0: flagged) as ((16 words, inf), (16 words, inf))"""
    xy, inf = points([(a + w * b) % R, (a - w * b) % R], FORM_STD if out_std else FORM_MONT, fill=0)
    return (xy[0], inf[0]), (xy[1], inf[1])


def srs_sets():
    """tests/golden/srs_kzg_points.json: (file, k, omega, g [2^k x 16], g_lagrange [2^k x 16]) of the halo2 KZG parameter files, arkworks
    Montgomery words as stored: g[j] = tau^j * G and g_lagrange[i] = L_i(tau) * G of one tau nobody knows"""
    d = json.load(open(os.path.join(ROOT, "tests", "golden", "srs_kzg_points.json")))
    pts = lambda hexes: np.stack([np.frombuffer(bytes.fromhex(h), dtype="<u4") for h in hexes]).astype(np.uint32)  # noqa: E731
    return [(st["file"], st["k"], int(st["omega_hex"], 16), pts(st["g_mont_le_hex"]), pts(st["g_lagrange_mont_le_hex"])) for st in d["sets"]]


def point_ints(rec):
    return orc.words_to_int(rec[:8]), orc.words_to_int(rec[8:])
