"""Inputs and expected values of the G2 group transform's tests (tests/test_g2_fft_cpu.py, tests/test_gpu_19_g2_fft.py) and of
tools/g2_fft_timing.py: points Q_j = a_j * H from seeded logarithms, the expected transform as the points of the Fr transform of the a_j in
Python integers -- the logarithms, that transform, the structured vectors, the edge twiddles and the flag matrix are those of the G1 tests
(tools/g1_fft_cases.py, imported as they are); the points come from the model of tools/fixed_base_g2_cases.py, which is built on the independent
Python G2 law of tools/bn254_g2_py.py.  A flagged place carries garbage words.  Nothing here touches the code under test."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import bn254_g2_py as g2  # noqa: E402
import fixed_base_g2_cases as fb2  # noqa: E402
import g1_fft_cases as g1c  # noqa: E402
import g2_pointwise_mul_cases as pm2  # noqa: E402

P, R = g2.P, g2.R
assert (P, R) == (g1c.P, g1c.R)
FORM_STD, FORM_MONT = g1c.FORM_STD, g1c.FORM_MONT
INVERSE, OUT_STD, IN_STD = g1c.INVERSE, g1c.OUT_STD, g1c.IN_STD
FLAG_MATRIX = g1c.FLAG_MATRIX
GARBAGE = g1c.GARBAGE
GEN = g2.G2_GEN
root, logs, transform_logs, identity_cases, edge_twiddles = g1c.root, g1c.logs, g1c.transform_logs, g1c.identity_cases, g1c.edge_twiddles


def points(a, form=FORM_MONT):
    """(n x 32 words, n bytes) of the points a_j * H: a_j = 0 (mod r) is flagged and its words are GARBAGE"""
    pts = fb2.points([v % R for v in a], GEN)
    xy = pm2.point_array(pts, form)
    inf = np.array([1 if pt is None else 0 for pt in pts], np.uint8)
    xy[inf != 0] = GARBAGE
    return xy, inf


def inputs(a, flags=0):
    return points(a, FORM_STD if flags & IN_STD else FORM_MONT)


def expected(a, log_n, flags=0, batch=1):
    """(points x 32 words, bytes) the call must leave for the inputs a_j * H: the points of the transformed logarithms in the requested form, 32
    zero words and inf = 1 where the logarithm is 0"""
    return fb2.expected(transform_logs(a, log_n, bool(flags & INVERSE), batch), GEN, bool(flags & OUT_STD))


def butterfly_expected(a, b, w, out_std=False):
    """(A + w B, A - w B) for A = a * H, B = b * H (0: flagged) as ((32 words, inf), (32 words, inf))"""
    xy, inf = fb2.expected([(a + w * b) % R, (a - w * b) % R], GEN, out_std)
    return (xy[0], inf[0]), (xy[1], inf[1])


def point_ints(rec):
    """the four integers of a record of 32 words"""
    return pm2.point_ints(rec)
