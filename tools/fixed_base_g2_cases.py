"""Inputs and expected values of the G2 fixed-base multiplication's tests (tests/test_fixed_base_g2_cpu.py, tests/test_gpu_12_fixed_base_g2.py)
and of tools/fixed_base_g2_timing.py.  The expected values come from a model built on the independent Python law of tools/bn254_g2_py.py and
never on the library: an 8-bit UNSIGNED window table of the base made with batched affine additions (one Fq inversion per table level), and the
products of k reduced modulo r by one batched addition per window over all scalars at once.  g2.add steps in where an accumulator is still empty
or two x coordinates meet (a doubling or opposite points), which batch_add does not cover.  Scalar patterns and edge scalars are those of the G1
tests (tools/fixed_base_cases.py, imported as they are)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import bn254_g2_py as g2  # noqa: E402
import fixed_base_cases as fb  # noqa: E402

P, R = g2.P, g2.R
assert (P, R) == (fb.P, fb.R)
FORM_STD, FORM_MONT = 0, 1
GEN = g2.G2_GEN
MONT_R = fb.MONT_R
edge_scalars, patterns, to_words, words = fb.edge_scalars, fb.patterns, fb.to_words, fb.words
MODEL_BITS = 8
MODEL_WINDOWS = 32  # 254 bits of k mod r
_TABLES = {}


def base_words(pt, form=FORM_STD):
    """32 words x.c0, x.c1, y.c0, y.c1"""
    return np.array(g2.point_words(pt, form == FORM_MONT), np.uint32)


def _safe_add_all(ps, qs):
    """[p + q]: batch_add where it applies, g2.add for None operands and equal x"""
    out, bi = [None] * len(ps), []
    for i, (p, q) in enumerate(zip(ps, qs)):
        if p is None or q is None or p[0] == q[0]:
            out[i] = g2.add(p, q)
        else:
            bi.append(i)
    if bi:
        for i, s in zip(bi, g2.batch_add([ps[i] for i in bi], [qs[i] for i in bi])):
            out[i] = s
    return out


def table(base=GEN):
    """T[j][d] = d * 2^(8 j) * base for d = 0 .. 255 (T[j][0] = None), j < 32; made once per base"""
    if base in _TABLES:
        return _TABLES[base]
    firsts = [base]
    for _ in range(MODEL_WINDOWS - 1):
        q = firsts[-1]
        for _ in range(MODEL_BITS):
            q = g2.add(q, q)
        firsts.append(q)
    rows = [[None, f] for f in firsts]
    size = 1  # entries 1 .. size are there
    while size < (1 << MODEL_BITS) - 1:
        # entries size + 1 .. 2 size (+ 1): T[t] + T[size] for t = 1 .. size; t == size doubles
        ps, qs, where = [], [], []
        for j, row in enumerate(rows):
            for t in range(1, size + 1):
                if size + t < 1 << MODEL_BITS:
                    ps.append(row[t]), qs.append(row[size]), where.append(j)
        sums = _safe_add_all(ps, qs)
        for j, s in zip(where, sums):
            rows[j].append(s)
        size = len(rows[0]) - 1
    assert all(len(r) == 1 << MODEL_BITS for r in rows)
    _TABLES[base] = rows
    return rows


def points(ks, base=GEN):
    """[(k mod r) * base] as affine points, None for the identity"""
    t = table(base)
    ks = [k % R for k in ks]
    acc = [None] * len(ks)
    for j in range(MODEL_WINDOWS):
        idx = [i for i, k in enumerate(ks) if (k >> (MODEL_BITS * j)) & 0xFF]
        if not idx:
            continue
        sums = _safe_add_all([acc[i] for i in idx], [t[j][(ks[i] >> (MODEL_BITS * j)) & 0xFF] for i in idx])
        for i, s in zip(idx, sums):
            acc[i] = s
    return acc


def point(k, base=GEN):
    return points([k], base)[0]


def expected(ks, base=GEN, out_std=False):
    """(n x 32 words, n bytes) the call must give for the integers ks: canonical coordinates in the output form, zeros and inf = 1 for the identity"""
    pts = points(ks, base)
    xy, inf = np.zeros((len(ks), 32), np.uint32), np.zeros(len(ks), np.uint8)
    for i, pt in enumerate(pts):
        if pt is None:
            inf[i] = 1
        else:
            xy[i] = g2.point_words(pt, not out_std)
    return xy, inf


def off_subgroup_point(seed=7):
    """a point of the twist outside G2: a random twist point that the cofactor does not clear (the construction of tests/test_g2_points_cpu.py)"""
    import random
    rnd = random.Random(seed)
    while True:
        x = (rnd.randrange(P), rnd.randrange(P))
        y = g2.sqrt2(g2.add2(g2.mul2(g2.mul2(x, x), x), g2.B_TWIST))
        if y is None:
            continue
        pt = (x, y)
        if g2.mul_raw(pt, R) is not None:
            return pt
