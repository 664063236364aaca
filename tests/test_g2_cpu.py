"""BN254 G2 without a GPU: the independent Python group law, the zkey G2 fixtures, the host-side fold msm_bn254_g2_combine against the Python law,
the new C-ABI symbols, and the no-device error of the G2 call."""
import json
import os
import random
import sys

import numpy as np
import pytest

import mopro_msm_hip as mh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bn254_g2_py as g2  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
G = g2.G2_GEN


def zkey_points():
    with open(os.path.join(GOLDEN, "zkey_g2_points.json")) as f:
        pts = json.load(f)["points"]
    out = []
    for p_ in pts:
        ws = np.frombuffer(bytes.fromhex(p_["mont_le_hex"]), "<u4")
        out.append((p_, None if p_["infinity"] else g2.jacobian_mont_to_affine(list(ws) + g2.jacobian_mont_words(G)[32:48])))
    return out


# ---- the Python law itself ------------------------------------------------------------------------------------------------------
def test_generator_on_twist_and_of_order_r():
    assert g2.on_curve(G)
    assert g2.mul_raw(G, g2.R) is None
    assert g2.mul_raw(G, g2.R - 1) == g2.neg(G)
    assert g2.add(g2.mul(G, 5), g2.mul(G, 7)) == g2.mul(G, 12)


def test_endomorphism_is_lambda_with_beta_squared():
    lam, beta = g2.glv_lambda_beta()
    b2 = beta * beta % g2.P
    assert b2 == (g2.P - beta - 1) % g2.P
    for k in (1, 3, 0x1234567):
        p_ = g2.mul(G, k)
        assert g2.mul(p_, lam) == (g2.smul2(p_[0], b2), p_[1])


def test_endomorphism_matches_the_split_lambda():
    """the planner's split writes k = k1 + lambda * k2 with lambda of tests/golden/glv_constants.json: phi2 = (beta^2 x, y) must be THAT lambda"""
    with open(os.path.join(GOLDEN, "glv_constants.json")) as f:
        c = json.load(f)
    lam = int(c["lambda"], 16)
    beta = int(c["beta"], 16) if "beta" in c else None
    p_ = g2.mul(G, 99)
    img = g2.mul(p_, lam)
    assert img[1] == p_[1]
    if beta is not None:
        assert img[0] == g2.smul2(p_[0], beta * beta % g2.P)


def test_zkey_g2_fixtures_on_twist_and_in_g2():
    pts = zkey_points()
    names = [p_["section"] for p_, _ in pts]
    assert names.count("B2") == 4 and {"beta2", "gamma2", "delta2"} <= set(names)
    assert sum(1 for p_, a in pts if p_["section"] == "B2" and a is None) == 3
    for p_, a in pts:
        if a is not None:
            assert g2.on_curve(a) and g2.mul_raw(a, g2.R) is None, p_["section"]


def test_g2_goldens_are_consistent():
    with open(os.path.join(GOLDEN, "g2_index.json")) as f:
        vecs = json.load(f)["vectors"]
    assert len(vecs) >= 13
    g = np.load(os.path.join(GOLDEN, "msm_g2_rand_n3.npz"))
    pts = [((g2.words_int(b[0:8]), g2.words_int(b[8:16])), (g2.words_int(b[16:24]), g2.words_int(b[24:32]))) for b in g["bases"]]
    sc = [g2.words_int(s) for s in g["scalars"]]
    assert all(g2.on_curve(p_) for p_ in pts)
    assert g2.affine_words_std(g2.msm(pts, sc)) == g["expected"].tolist()


# ---- msm_bn254_g2_combine (host arithmetic of the product) against the Python law ------------------------------------------------
def jac_words(pt, rnd):
    """pt with a random Z (not 1): the fold must not depend on the representative"""
    z = (rnd.randrange(1, g2.P), rnd.randrange(g2.P))
    return g2.jacobian_mont_words(pt, z)


@pytest.mark.parametrize("flags", [0, mh.FLAG_DETERMINISTIC])
@pytest.mark.parametrize("case", ["k1", "k2", "k5", "identity", "p_minus_p", "p_plus_p"])
def test_combine_g2_against_python(case, flags):
    rnd = random.Random(hash(case) & 0xFFFF)
    a, b = g2.mul(G, 11), g2.mul(G, 0xABCDEF)
    pts = {"k1": [a], "k2": [a, b], "k5": [g2.mul(G, rnd.randrange(1, g2.R)) for _ in range(5)], "identity": [None, a, None],
           "p_minus_p": [a, g2.neg(a)], "p_plus_p": [b, b]}[case]
    exp = None
    for p_ in pts:
        exp = g2.add(exp, p_)
    parts = np.array([jac_words(p_, rnd) if p_ is not None else g2.jacobian_mont_words(None) for p_ in pts], np.uint32)
    r = mh.combine_partials_g2(parts, flags=flags)
    assert r.is_infinity == (exp is None)
    assert r.affine_std.tolist() == g2.affine_words_std(exp)
    assert g2.jacobian_mont_to_affine(r.jacobian_mont.tolist()) == exp
    if exp is not None:
        assert r.affine_ints() == exp
    if flags & mh.FLAG_DETERMINISTIC:
        assert r.jacobian_mont.tolist() == g2.jacobian_mont_words(exp)  # the Z = 1 representative, (1, 1, 0) for the identity


def test_combine_g2_errors():
    lib = mh.load_library()
    out = np.zeros(48, np.uint32)
    parts = np.array([g2.jacobian_mont_words(G)], np.uint32)
    assert lib.msm_bn254_g2_combine(None, 1, 0, mh._p32(out), None, None) == mh.ERR_BAD_ARG
    assert lib.msm_bn254_g2_combine(mh._p32(parts), 0, 0, mh._p32(out), None, None) == mh.ERR_EMPTY
    assert lib.msm_bn254_g2_combine(mh._p32(parts), 1, mh.FLAG_NO_GLV, mh._p32(out), None, None) == mh.ERR_BAD_ARG
    with pytest.raises(mh.MsmError):
        mh.combine_partials_g2(np.zeros((0, 48), np.uint32))


# ---- the ABI --------------------------------------------------------------------------------------------------------------------
def test_library_exports_g2_symbols():
    lib = mh.load_library()
    for name in ("msm_bn254_g2", "msm_bn254_g2_device", "msm_bn254_g2_combine"):
        assert name in mh.ABI_SYMBOLS
        assert getattr(lib, name) is not None
    hdr = open(os.path.join(ROOT, "include", "msm_hip.h")).read()
    assert "out_jacobian_mont[48]" in hdr and "#define MSM_HIP_ABI_VERSION 7" in hdr


def test_g2_call_null_context_is_bad_arg():
    lib = mh.load_library()
    b, s = np.zeros(32, np.uint32), np.zeros(8, np.uint32)
    assert lib.msm_bn254_g2(None, mh._p32(b), 0, None, mh._p32(s), 1, None, None, None) == mh.ERR_BAD_ARG
    assert lib.msm_bn254_g2_device(None, b.ctypes.data, None, s.ctypes.data, 1, None, None, None, None) == mh.ERR_BAD_ARG


def _have_gpu():
    try:
        import torch
        return torch.cuda.is_available() and torch.cuda.device_count() > 0
    except Exception:
        return False


@pytest.mark.skipif(_have_gpu(), reason="a GPU is present: the no-device error cannot be observed")
def test_g2_without_gpu_raises_no_device():
    g = np.load(os.path.join(GOLDEN, "msm_g2_rand_n2.npz"))
    with pytest.raises(mh.MsmError) as e:
        mh.hip_variable_base_msm_g2(g["bases"], g["scalars"])
    assert e.value.code == mh.ERR_NO_DEVICE


def test_product_never_imports_the_g2_checker():
    pkg = os.path.join(ROOT, "gpu-acceleration_amd")
    for dirpath, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith((".py", ".hpp", ".hip", ".inc", ".h")):
                assert "bn254_g2_py" not in open(os.path.join(dirpath, fn), errors="replace").read(), fn
