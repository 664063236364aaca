"""Decoding and validating BN254 G2 points, without a GPU: the independent Python statement of the checks (tools/bn254_g2_py.py: Fq2 square roots,
the compressed image format, psi, the defining subgroup test), the goldens of tools/gen_golden_g2_compressed.py, the host-only
msm_bn254_g2_compress against the Python compress, the new C-ABI symbols and their argument errors."""
import ctypes as C
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import mopro_msm_hip as mh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bn254_g2_py as g2  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
P, R, G = g2.P, g2.R, g2.G2_GEN
X_BN = 4965661367192848881
HIPCC = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"  # what csrc/Makefile builds the product with: no hipcc, no product
NEW_SYMBOLS = ["msm_bn254_g2_compress", "msm_bn254_g2_decompress", "msm_bn254_g2_decompress_device", "msm_bn254_g2_validate",
               "msm_bn254_g2_validate_device", "msm_bn254_g1_validate"]


def goldens():
    with open(os.path.join(GOLDEN, "g2_compressed_points.json")) as f:
        return json.load(f)


def mont_words(hexstr):
    return np.frombuffer(bytes.fromhex(hexstr), "<u4").astype(np.uint32)


def point_of(entry):
    """the affine point of a golden entry's Montgomery words (None for infinity)"""
    if entry.get("infinity") or entry["mont_le_hex"] is None:
        return None
    v = g2.from_mont_words(mont_words(entry["mont_le_hex"]).tolist())
    return ((v[0], v[1]), (v[2], v[3]))


def shortcut_relation(pt):
    """the relation the kernel evaluates instead of [r]P: [x+1]P + psi([x]P) + psi^2([x]P) == psi^3([2x]P)"""
    xp = g2.mul_raw(pt, X_BN)
    lhs = g2.add(g2.add(g2.add(xp, pt), g2.psi(xp)), g2.psi(g2.psi(xp)))
    return lhs == g2.psi(g2.psi(g2.psi(g2.add(xp, xp))))


# ---- the Python law's own checks ------------------------------------------------------------------------------------------------
def test_psi_is_multiplication_by_p_on_g2():
    assert g2.psi(G) == g2.mul(G, P % R)
    q = g2.mul(G, 0xABCDEF0123)
    assert g2.psi(q) == g2.mul(q, P % R) and g2.on_curve(g2.psi(q))
    assert g2.psi(None) is None


def test_fq2_sqrt_round_trips():
    rnd = random.Random(1)
    vals = [(rnd.randrange(P), rnd.randrange(P)) for _ in range(40)] + [(rnd.randrange(P), 0), (0, rnd.randrange(P)), (0, 0), (1, 0), (P - 1, 0)]
    squares = 0
    for a in vals:
        sq = g2.mul2(a, a)
        r = g2.sqrt2(sq)
        assert r in (a, g2.neg2(a))
        r = g2.sqrt2(a)
        if r is not None:
            squares += 1
            assert g2.mul2(r, r) == a
        else:
            assert g2.pow2(a, (P * P - 1) // 2) == (P - 1, 0)  # Euler: no square
    assert 5 < squares < len(vals)
    assert g2.pow2((3, 4), 5) == g2.mul2(g2.mul2(g2.mul2((3, 4), (3, 4)), g2.mul2((3, 4), (3, 4))), (3, 4))


def test_order_of_fq2_is_c1_first():
    assert g2.is_larger2((0, 1)) is False and g2.is_larger2((0, P - 1)) is True      # c1 decides
    assert g2.is_larger2((P - 1, 1)) is False and g2.is_larger2((1, P - 1)) is True  # ... whatever c0 is
    assert g2.is_larger2((P - 1, 0)) is True and g2.is_larger2((1, 0)) is False      # c1 = 0: c0 decides
    assert g2.is_larger2((0, 0)) is False
    assert g2.is_larger2(((P - 1) // 2, 0)) is False and g2.is_larger2(((P + 1) // 2, 0)) is True


def test_subgroup_verdicts_defining_and_shortcut():
    gd = goldens()
    assert g2.COFACTOR % (10069 * 5864401 * 1875725156269) == 0
    for e in gd["valid"]:
        pt = point_of(e)
        assert g2.in_subgroup(pt)
        if pt is not None:
            assert g2.on_curve(pt) and shortcut_relation(pt), e["name"]
    sub = [e for e in gd["invalid"] if e["reason"] == "subgroup"]
    assert {e["name"] for e in sub} == {"random_twist_point", "order_10069", "order_5864401", "g2_plus_order_10069"}
    for e in sub:
        pt = point_of(e)
        assert g2.on_curve(pt) and not g2.in_subgroup(pt) and not shortcut_relation(pt), e["name"]
        cleared = g2.mul_raw(pt, g2.COFACTOR)  # [2p - r]Q lies in G2
        assert g2.in_subgroup(cleared) and (cleared is None or shortcut_relation(cleared))
    by = {e["name"]: point_of(e) for e in sub}
    assert g2.mul_raw(by["order_10069"], 10069) is None and g2.mul_raw(by["order_5864401"], 5864401) is None


def test_goldens_decode_in_python():
    gd = goldens()
    assert len(gd["valid"]) >= 12 and sum(e["infinity"] for e in gd["valid"]) >= 3
    assert {e["larger_y"] for e in gd["valid"] if not e["infinity"]} == {True, False}
    for e in gd["valid"]:
        img = bytes.fromhex(e["image_hex"])
        pt = g2.decompress(img)
        assert pt == point_of(e) and g2.compress(pt) == img
        assert mont_words(e["mont_le_hex"]).tolist() == g2.point_words(pt, mont=True)
    reasons = {e["name"]: e["reason"] for e in gd["invalid"]}
    assert reasons["both_flags"] == reasons["c0_ge_p"] == reasons["c1_ge_p"] == "decode" and reasons["non_residue_x"] == "curve"
    for e in gd["invalid"]:
        img = bytes.fromhex(e["image_hex"])
        if e["reason"] == "subgroup":
            assert g2.decompress(img) == point_of(e)
        else:
            with pytest.raises(ValueError) as err:
                g2.decompress(img)
            assert str(err.value) == e["reason"]
    c1 = int.from_bytes(bytes.fromhex([e for e in gd["invalid"] if e["name"] == "c1_ge_p"][0]["image_hex"])[32:], "little")
    assert P <= c1 < 1 << 254  # needs no flag bit to be >= p


# ---- msm_bn254_g2_compress (host code of the product) against the Python compress ------------------------------------------------
def golden_bases():
    gd = goldens()
    ents = gd["valid"] + [e for e in gd["invalid"] if e["reason"] == "subgroup"]  # (compress does not validate)
    pts = [point_of(e) for e in ents]
    imgs = b"".join(bytes.fromhex(e["image_hex"]) for e in ents)
    mont = np.array([g2.point_words(p_, mont=True) for p_ in pts], np.uint32)
    std = np.array([g2.point_words(p_, mont=False) for p_ in pts], np.uint32)
    inf = np.array([p_ is None for p_ in pts], np.uint8)
    return pts, imgs, mont, std, inf


def test_compress_matches_python_both_forms():
    pts, imgs, mont, std, inf = golden_bases()
    assert inf.any() and not inf.all()
    assert mh.compress_points_g2(mont, mh.FORM_MONT, inf) == imgs
    assert mh.compress_points_g2(std, mh.FORM_STD, inf) == imgs
    keep = np.flatnonzero(inf == 0)
    assert mh.compress_points_g2(std[keep], mh.FORM_STD) == b"".join(g2.compress(pts[i]) for i in keep)
    # the mask wins over whatever the coordinates are
    assert mh.compress_points_g2(std[keep[:2]], mh.FORM_STD, np.array([1, 0], np.uint8)) == g2.compress(None) + g2.compress(pts[keep[1]])


def test_compress_sign_rule_on_constructed_y():
    """the image only depends on x and the ORDER of y: y values with a zero component exercise the c1 = 0 / c0 = 0 branches (compress does not check
    the curve equation)"""
    x = (5, 7)
    for y in ((0, 1), (0, P - 1), (1, 0), (P - 1, 0), ((P - 1) // 2, 0), ((P + 1) // 2, 0), (9, (P - 1) // 2), (9, (P + 1) // 2), (0, 0), (P - 1, 1), (1, P - 1)):
        for mont in (False, True):
            w = np.array([g2.point_words((x, y), mont=mont)], np.uint32)
            assert mh.compress_points_g2(w, mh.FORM_MONT if mont else mh.FORM_STD) == g2.compress((x, y)), (y, mont)


def test_compress_many_points_threads():
    pts = g2.chain_points(3, 5, 64)
    w = np.array([g2.point_words(p_, mont=True) for p_ in pts], np.uint32)
    n = 20000  # above the single-thread limit of the host loop
    big = np.ascontiguousarray(np.tile(w, (n // 64 + 1, 1))[:n])
    inf = (np.arange(n) % 7 == 0).astype(np.uint8)
    img = mh.compress_points_g2(big, mh.FORM_MONT, inf)
    exp = [g2.compress(p_) for p_ in pts]
    assert len(img) == 64 * n
    assert all(img[64 * i:64 * i + 64] == (g2.compress(None) if inf[i] else exp[i % 64]) for i in range(n))


def test_compress_argument_errors():
    lib = mh.load_library()
    w, out = np.zeros((1, 32), np.uint32), np.zeros(64, np.uint8)
    u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
    assert lib.msm_bn254_g2_compress(None, 0, None, 1, u8(out)) == mh.ERR_BAD_ARG
    assert lib.msm_bn254_g2_compress(mh._p32(w), 0, None, 1, None) == mh.ERR_BAD_ARG
    assert lib.msm_bn254_g2_compress(mh._p32(w), 2, None, 1, u8(out)) == mh.ERR_BAD_ARG
    assert lib.msm_bn254_g2_compress(mh._p32(w), 0, None, 0, u8(out)) == mh.ERR_EMPTY
    assert lib.msm_bn254_g2_compress(mh._p32(w), 0, None, 1, u8(out)) == mh.OK
    with pytest.raises(mh.MsmError) as e:
        mh.compress_points_g2(np.zeros((0, 32), np.uint32))
    assert e.value.code == mh.ERR_EMPTY


# ---- the kernels' own arithmetic on the CPU, every limb bound asserted ----------------------------------------------------------
def test_kernel_arithmetic_on_the_host_with_bounds_checked(tmp_path):
    """gpu-acceleration_amd/csrc/g2_points_bn254.hpp is __host__ __device__: tools/g2_points_check.cpp runs the root-and-sign routine, the curve
    equation and the subgroup test of the kernels on the CPU with -DFP_BOUNDS_CHECK, and every answer must be the Python law's"""
    exe = tmp_path / "g2_points_check"
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-DFP_BOUNDS_CHECK", "-x", "hip", "--cuda-host-only",  # host code only: no device pass
                    os.path.join(ROOT, "tools", "g2_points_check.cpp"), "-o", str(exe)], check=True, capture_output=True, timeout=900)
    h = lambda v: "%064x" % v
    rnd = random.Random(5)
    vals = [g2.mul2(t, t) for t in [(rnd.randrange(P), rnd.randrange(P)) for _ in range(40)]]  # squares
    vals += [(rnd.randrange(1, P), 0) for _ in range(40)]                                       # Fq: residues (c1 = 0 roots) and non-residues (c0 = 0 roots)
    vals += [(0, rnd.randrange(P)) for _ in range(8)] + [(0, 0), (1, 0), (P - 1, 0), (0, 1), (0, P - 1)]
    vals += [(rnd.randrange(P), rnd.randrange(P)) for _ in range(40)]                           # about half of them no squares
    roots = [g2.sqrt2(v) for v in vals]
    assert any(r is not None and r[1] == 0 and r[0] for r in roots) and any(r is not None and r[0] == 0 and r[1] for r in roots)
    assert any(r is None for r in roots) and any(g2.pow2(v, (P - 1) // 2) == (P - 1, 0) for v in vals)
    queries, expect = [], []
    for v, r in zip(vals, roots):
        for want in (0, 1):
            queries.append("S %s %s %d" % (h(v[0]), h(v[1]), want))
            if r is None:
                expect.append("S 0 %s %s" % (h(0), h(0)))
            else:
                y = g2.neg2(r) if r != (0, 0) and g2.is_larger2(r) != bool(want) else r
                expect.append("S 1 %s %s" % (h(y[0]), h(y[1])))
    gd = goldens()
    pts = [point_of(e) for e in gd["valid"] + gd["invalid"]]
    pts += [g2.mul_raw(point_of(e), g2.COFACTOR) for e in gd["invalid"] if e["reason"] == "subgroup"]  # cleared of the cofactor: in G2 (or O)
    pts = [p_ for p_ in pts if p_ is not None]
    assert sum(not g2.in_subgroup(p_) for p_ in pts) == 4
    for p_ in pts:
        c = (p_[0][0], p_[0][1], p_[1][0], p_[1][1])
        queries.append("P " + " ".join(h(v) for v in c))
        expect.append("P 1 %d" % g2.in_subgroup(p_))
        queries.append("P " + " ".join(h(v) for v in (c[0], c[1], c[2], (c[3] + 1) % P)))  # off the twist
        expect.append("P 0 0")
    r = subprocess.run([str(exe)], input="\n".join(queries) + "\n", capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "%d queries, no bound violated" % len(queries)
    assert lines[:-1] == expect


def test_no_new_kernel_uses_scratch_memory(tmp_path):
    """The subgroup test only stays out of scratch memory because its repeated operand is hidden from the optimiser (g2_points_bn254.hpp g2p_opaque),
    and the window multiplication of the square root because it is a switch: a compiler that undoes either brings kilobytes of scratch per lane
    back silently.  The kernels are compiled alone for gfx950 and the compiler's own resource remarks are read."""
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-DMSM_HIP_TEST_HOOKS", "--cuda-device-only", "-c", "-o", str(tmp_path / "k.o"),
                        os.path.join(ROOT, "tools", "g2_points_resource_check.hip"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stderr[-3000:]
    import re
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == 5, names
    for want in ("k_g2_decompressILb0", "k_g2_decompressILb1", "k_g2_validate", "k_g1_validate", "k_g2_test_sqrt"):
        assert any(want in n for n in names), (want, names)
    assert all(v == 0 for v in scratch), dict(zip(names, scratch))


# ---- the ABI --------------------------------------------------------------------------------------------------------------------
def test_new_symbols_exported_and_bound():
    lib = mh.load_library()
    hdr = open(os.path.join(ROOT, "include", "msm_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in mh.ABI_SYMBOLS and getattr(lib, name) is not None
        assert getattr(lib, name).argtypes is not None and name + "(" in hdr
    assert mh.G2_CHECK_CURVE == 1 and mh.G2_CHECK_SUBGROUP == 2
    assert "#define MSM_G2_CHECK_CURVE    1u" in hdr and "#define MSM_G2_CHECK_SUBGROUP 2u" in hdr and "#define MSM_HIP_ABI_VERSION 7u" in hdr
    for meth in ("decompress_g2", "decompress_g2_device", "validate_g2", "validate_g2_device", "validate_g1"):
        assert callable(getattr(mh.MsmContext, meth))


def test_hook_lives_in_the_hooks_build_only():
    from mopro_msm_hip import testhooks as th
    assert "msm_test_g2_sqrt" in th.HOOK_SYMBOLS
    assert hasattr(th.load_hooks_library(), "msm_test_g2_sqrt") and not hasattr(mh.load_library(), "msm_test_g2_sqrt")


def test_null_context_is_bad_arg_on_every_gpu_call():
    lib = mh.load_library()
    img, xy, inf, w = np.zeros(64, np.uint8), np.zeros(32, np.uint32), np.zeros(1, np.uint8), np.zeros(32, np.uint32)
    u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
    bad = C.c_int64(5)
    S = mh.G2_CHECK_SUBGROUP
    assert lib.msm_bn254_g2_decompress(None, u8(img), 1, 0, mh._p32(xy), u8(inf), C.byref(bad)) == mh.ERR_BAD_ARG
    assert lib.msm_bn254_g2_decompress_device(None, u8(img), 1, S, xy.ctypes.data, inf.ctypes.data, None, None) == mh.ERR_BAD_ARG
    assert lib.msm_bn254_g2_validate(None, mh._p32(w), mh.FORM_MONT, None, 1, S, None) == mh.ERR_BAD_ARG
    assert lib.msm_bn254_g2_validate_device(None, w.ctypes.data, None, 1, S, None, None) == mh.ERR_BAD_ARG
    assert lib.msm_bn254_g1_validate(None, mh._p32(w), mh.FORM_MONT, None, 1, None) == mh.ERR_BAD_ARG


def _have_gpu():
    try:
        import torch
        return torch.cuda.is_available() and torch.cuda.device_count() > 0
    except Exception:
        return False


def test_without_gpu_context_creation_still_raises_no_device():
    if _have_gpu():
        with mh.MsmContext() as c:  # with one, the calls exist on a context and refuse an empty input before touching the device
            with pytest.raises(mh.MsmError) as e:
                c.decompress_g2(b"")
            assert e.value.code == mh.ERR_EMPTY
        return
    with pytest.raises(mh.MsmError) as e:
        mh.MsmContext()
    assert e.value.code == mh.ERR_NO_DEVICE
