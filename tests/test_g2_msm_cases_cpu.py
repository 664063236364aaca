"""The yardstick of tests/test_gpu_18_g2_msm_degenerate.py checked without a GPU: every shape of tools/g2_msm_cases.py at n <= 24 -- the closed form
(sum s_i c_i mod r) * G2 against g2.msm over the affine points decoded back from the emitted words, in both forms and under a mask; every emitted
base on the curve; the endomorphism (phi2(P) = lambda * P, P + phi2(P) + phi2^2(P) = O, beta^2 as the kernels' header spells it); the word
images of negated points; and the bookkeeping that says which list of the combine kernel a bucket reaches."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bn254_g2_py as g2  # noqa: E402
import g2_msm_cases as gc  # noqa: E402

P, R = g2.P, g2.R
FORMS = (gc.FORM_STD, gc.FORM_MONT)


def small_shapes():
    """(label, Instance) of every shape at n <= 24"""
    # (one scalar multiplication of the Python law takes ~50 ms: the sizes are as small as the shapes allow, one of them at 24)
    out = [("tiled(3, 8)", gc.raw_tiled(3, 8, 11)), ("tiled(3, 2) spread", gc.raw_tiled(3, 2, 12, gc.spread_scalars(12))),
           ("tiled(1, 2)", gc.raw_tiled(1, 2, 13)), ("opposite(2, 2)", gc.raw_opposite(2, 2, 14)),
           ("opposite(2, 2) + 1", gc.raw_opposite(2, 2, 15, extra=1)), ("opposite(2, 1) + 1 spread", gc.raw_opposite(2, 1, 16, 1, gc.spread_scalars(16)[:2])),
           ("scalar_opposite(4)", gc.raw_scalar_opposite(4, 17)), ("endo_triple(1)", gc.raw_endo_triple(1, 18)),
           ("endo_triple(3)", gc.raw_endo_triple(3, 19)), ("endo_triple(1) distinct", gc.raw_endo_triple(1, 20, True)),
           ("endo_triple(3) distinct", gc.raw_endo_triple(3, 21, True))]
    for m in (2, 3, 24):
        for sign in ("same", "alt"):
            out.append((f"one_base_ramp({m}, 8, {sign})", gc.raw_one_base_ramp(m, 8, sign)))
    out += [("mask " + lbl, gc.raw_with_mask(inst, 40 + i)) for i, (lbl, inst) in enumerate(list(out)) if inst.n >= 6 and "tiled(3, 8)" not in lbl]
    # the net: every combination, at a size that still shows its base mode (odd rows: 2, every third: 3, all equal: 4), the last eight larger
    out += [("net %d: %s" % (it, combo), inst) for it in range(gc.NET_CASES) for combo, inst in [gc.net_case(it, n=(1 if it < 32 else 9) + it % 4)]]
    return out


def check_instance(label, inst):
    assert 1 <= inst.n <= 24, label
    exp = inst.expected()
    decoded = []
    for form in FORMS:
        bases, scalars, inf, e = inst.emit(form)
        assert bases.shape == (inst.n, 32) and scalars.shape == (inst.n, 8) and bases.dtype == scalars.dtype == np.uint32, label
        assert e == exp and (inf is None or (inf.shape == (inst.n,) and inf.dtype == np.uint8)), label
        pts = gc.decode(bases, form)
        sc = [g2.words_int(row) for row in scalars]
        assert all(s < R for s in sc), label
        live = [i for i in range(inst.n) if inf is None or not inf[i]]
        assert all(pts[i] is not None and g2.on_curve(pts[i]) for i in live), label          # every base the call may read as a point
        assert all(p_ is None or g2.on_curve(p_) for p_ in pts), label                        # masked rows: zeros or the point
        decoded.append((pts, sc, live))
    assert decoded[0] == decoded[1], label                                                    # both forms hold the same instance ...
    pts, sc, live = decoded[0]
    assert g2.msm([pts[i] for i in live], [sc[i] for i in live]) == exp, label                # ... whose sum by the independent law, term by term
    i = (7 * len(label)) % inst.n  # the logarithms are what the words hold (a spot row: one scalar multiplication)
    if pts[i] is not None:
        assert g2.mul(gc.GEN, inst.ulogs[inst.pidx[i]]) == pts[i], (label, i)


def test_every_shape_closed_form_equals_the_independent_msm():
    shapes = small_shapes()
    assert len(shapes) > 60 and max(inst.n for _, inst in shapes) == 24
    for label, inst in shapes:
        check_instance(label, inst)


def test_shapes_are_what_they_claim():
    b, s, inf, e = gc.tiled(3, 8, 11)
    assert (b[:3] == b[21:]).all() and (s[:3] == s[3:6]).all() and inf is None and e is not None and len({r.tobytes() for r in b}) == 3
    for T in (2, 5):
        b, s, inf, e = gc.opposite(3, T, 14)
        assert e is None and b.shape[0] == 6 * T
        b, s, inf, e = gc.opposite(3, T, 14, extra=1)
        assert b.shape[0] == 6 * T + 3
        lg, pts = gc.base_points(3, 14)
        assert e == g2.msm(pts, gc.seeded_scalars(14, 3))  # each bucket ends at P_j: the instance is sum s_j P_j
    b, s, inf, e = gc.scalar_opposite(12, 17)
    sc = [g2.words_int(r) for r in s]
    assert e is None and all((sc[j] + sc[12 + j]) % R == 0 and sc[j] != sc[12 + j] for j in range(12)) and (b[:12] == b[12:]).all()
    assert gc.endo_triple(8, 19)[3] is None and gc.endo_triple(8, 21, distinct=True)[3] is not None
    for sign, tot in (("same", 24 * 25 // 2), ("alt", -12)):
        b, s, inf, e = gc.one_base_ramp(24, 8, sign)
        assert [g2.words_int(r) for r in s] == list(range(1, 25)) and e == g2.mul(gc.GEN, tot * gc.RAMP_LOG % R)
        assert len({r.tobytes() for r in b}) == (1 if sign == "same" else 2)
    b, s, inf, e = gc.with_mask(gc.raw_opposite(3, 5, 22), 23)
    sc = [g2.words_int(r) for r in s]
    assert inf.any() and not inf.all() and any(v == 0 and not m for v, m in zip(sc, inf)) and any(not r.any() for r in b[inf == 1])
    assert any(r.any() for r in b[inf == 1])
    # the full-size fixture shape comes from the chain: logarithms a + i d
    lg, pts = gc.base_points(gc.CHAIN_FROM, 5)
    assert len(set(lg)) == gc.CHAIN_FROM and all(g2.mul(gc.GEN, lg[i]) == pts[i] for i in (0, 1, gc.CHAIN_FROM - 1))


def test_endomorphism_and_the_headers_beta2():
    # g2.glv_lambda_beta() pairs ITS lambda with ITS beta on G1; which of the two cube roots mod r goes with x -> BETA2 * x on G2 is settled by
    # the law itself (gc.lam()), not by the names
    l1, b1 = g2.glv_lambda_beta()
    lam = gc.lam()
    assert lam in (l1, l1 * l1 % R) and gc.BETA2 in (b1, b1 * b1 % P) and lam != 1 and pow(lam, 3, R) == 1 and (1 + lam + lam * lam) % R == 0
    assert gc.BETA2 != 1 and pow(gc.BETA2, 3, P) == 1
    import g2_pointwise_mul_cases as pm2
    assert (gc.BETA2, lam) == (pm2.BETA2, pm2.LAMBDA)  # the constants the element-wise multiplication's tests derive from tests/golden/glv_constants.json
    hdr = open(os.path.join(ROOT, "gpu-acceleration_amd", "csrc", "msm_kernels_g2.hpp")).read()
    m = re.search(r"BETA2_STD\[8\]\s*=\s*\{([^}]*)\}", hdr)
    assert g2.words_int([int(w.strip().rstrip("u"), 16) for w in m.group(1).split(",")]) == gc.BETA2
    for c in (1, 2, gc.RAMP_LOG, R - 1):
        pt = g2.mul(gc.GEN, c)
        p1, p2 = gc.phi2(pt), gc.phi2(gc.phi2(pt))
        assert g2.on_curve(p1) and p1 == g2.mul(pt, lam) and p2 == g2.mul(pt, lam * lam % R) and gc.phi2(p2) == pt
        assert g2.add(g2.add(pt, p1), p2) is None
    assert gc.phi2(None) is None


def test_word_images_of_negated_points():
    lg, pts = gc.base_points(4, 31)
    negs = [g2.neg(p_) for p_ in pts]
    for form in FORMS:
        w, wn = gc.point_array(pts, form), gc.point_array(negs, form)
        assert gc.decode(wn, form) == negs and (w[:, :16] == wn[:, :16]).all()
        for row, rown in zip(w, wn):  # y negated per Fq component, in the form's own domain
            for k in (2, 3):
                a, b = g2.words_int(row[8 * k:8 * k + 8]), g2.words_int(rown[8 * k:8 * k + 8])
                assert (a + b) % P == 0 and a < P and b < P
    b, s, inf, e = gc.opposite(4, 1, 31, form=gc.FORM_STD)
    assert gc.decode(b, gc.FORM_STD) == pts + negs


def test_spread_scalars_share_no_digit_at_any_width():
    for seed in range(6):
        sc = gc.spread_scalars(seed)
        assert len(set(sc)) == 3 and all(0 < s < 1 << gc.SPREAD_BITS for s in sc)
        for c in range(2, 21):  # every width the planner accepts; the top window (spread by point index) stays empty
            sizes = gc.unsigned_bucket_sizes(sc * 7, None, c)
            assert sizes and set(sizes.values()) == {7} and max(w for w, _ in sizes) < (254 + c - 1) // c - 1, (seed, c)
    sizes = gc.unsigned_bucket_sizes([5, 5, 6, 1 << 20], [0, 0, 0, 1], 8)
    assert dict(sizes) == {(0, 5): 2, (0, 6): 1}
    with pytest.raises(ValueError):
        gc.unsigned_bucket_sizes([1 << 250], None, 8)


@pytest.mark.parametrize("T,ell,want", [(2, 1, "mid2"), (5, 1, "mid"), (8, 1, "long"), (130, 1, "long"), (1100, 1, "long2"), (2, 2, None), (5, 2, "mid"),
                                        (8, 2, "mid"), (130, 2, "long"), (1100, 2, "long"), (2, 3, None), (5, 3, "mid2"), (8, 3, "mid"), (130, 3, "long"),
                                        (1100, 3, "long")])
def test_expected_lists_of_equal_buckets(T, ell, want):
    B = 37
    got = gc.expected_lists([T] * B, ell)
    m = -(-T // ell)
    assert got["pieces"] == (m if T > ell else 1) * B
    if want is None:
        assert got == dict(long=0, mid=0, pieces=B, partials=0, mid2=0)
    elif want == "mid2":
        assert m == 2 and got["mid2"] == B and got["mid"] == got["long"] == 0 and got["partials"] == 2 * B
    elif want == "mid":
        assert 3 <= m <= 7 and got["mid"] == B and got["mid2"] == got["long"] == 0 and got["partials"] == m * B
    elif want == "long":
        assert 8 <= m <= 1024 and got["long"] == B and got["mid"] == got["mid2"] == 0 and got["partials"] == m * got["long"]
    else:
        assert m == 1100 and got["long"] == 2 * B and 2 * got["partials"] == m * got["long"]
