"""Decoding and validating BN254 G2 points on the GPU (-m gpu): msm_bn254_g2_decompress(_device), msm_bn254_g2_validate(_device),
msm_bn254_g1_validate and the root-and-sign hook, against the independent Python law (tools/bn254_g2_py.py) and the goldens of
tools/gen_golden_g2_compressed.py.  Every comparison is word-exact."""
import json
import os
import random
import sys

import numpy as np
import pytest

import mopro_msm_hip as mh
from mopro_msm_hip import testhooks as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bn254_g2_py as g2  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden")
P, R, G = g2.P, g2.R, g2.G2_GEN
M = 1 << 18  # distinct bases of the large instances (the construction of test_gpu_7_g2.py)
A0, D0 = 0x1234567890ABCDEF1234567890ABCDEF, 0xFEDCBA987654321
CURVE, SUBGROUP = mh.G2_CHECK_CURVE, mh.G2_CHECK_SUBGROUP
WORDS = ("decode", "curve", "subgroup")


@pytest.fixture(scope="module")
def ctx():
    c = mh.MsmContext()
    yield c
    c.close()


@pytest.fixture(scope="module")
def big_bases():
    """(M x 32 standard-form words, M x 32 Montgomery words) of P_i = (A0 + i * D0) * G2"""
    pts = g2.chain_points(A0, D0, M)
    std = np.array([g2.point_words(p_) for p_ in pts], np.uint32)
    mont = np.array([g2.point_words(p_, mont=True) for p_ in pts], np.uint32)
    return std, mont


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(GOLDEN, "g2_compressed_points.json")) as f:
        return json.load(f)


def tile(arr, n):
    return np.ascontiguousarray(np.tile(arr, ((n + M - 1) // M, 1))[:n])


def mont_words(hexstr):
    return np.frombuffer(bytes.fromhex(hexstr), "<u4").astype(np.uint32)


def expect_invalid(call, index, word):
    with pytest.raises(mh.MsmError) as e:
        call()
    assert e.value.code == mh.ERR_INVALID_DATA
    assert e.value.first_invalid == index
    msg = str(e.value)
    assert word in msg and not any(w in msg for w in WORDS if w != word), msg


# 1. goldens through the host decompress
def test_goldens_valid_images_decode(ctx, gold):
    imgs = b"".join(bytes.fromhex(e["image_hex"]) for e in gold["valid"])
    want = np.stack([mont_words(e["mont_le_hex"]) for e in gold["valid"]])
    winf = np.array([e["infinity"] for e in gold["valid"]], np.uint8)
    for checks in (0, SUBGROUP):
        xy, inf = ctx.decompress_g2(imgs, checks)
        assert (xy == want).all() and (inf == winf).all(), checks
    for e in gold["valid"]:  # one at a time too
        xy, inf = ctx.decompress_g2(bytes.fromhex(e["image_hex"]), SUBGROUP)
        assert xy[0].tolist() == mont_words(e["mont_le_hex"]).tolist() and bool(inf[0]) == e["infinity"], e["name"]


def test_goldens_each_invalid_image_alone(ctx, gold):
    valid = [bytes.fromhex(e["image_hex"]) for e in gold["valid"]]
    want = np.stack([mont_words(e["mont_le_hex"]) for e in gold["valid"]])
    assert len(gold["invalid"]) >= 8
    for k, e in enumerate(gold["invalid"]):
        at = (5 * k + 3) % (len(valid) + 1)
        imgs = b"".join(valid[:at]) + bytes.fromhex(e["image_hex"]) + b"".join(valid[at:])
        expect_invalid(lambda: ctx.decompress_g2(imgs, SUBGROUP), at, e["reason"])
        if e["reason"] == "subgroup":  # only the subgroup test refuses it
            xy, inf = ctx.decompress_g2(imgs, 0)
            assert xy[at].tolist() == mont_words(e["mont_le_hex"]).tolist() and not inf.tolist()[at]
            assert (np.delete(xy, at, 0) == want).all()
        else:
            expect_invalid(lambda: ctx.decompress_g2(imgs, 0), at, e["reason"])


# 2. the lowest failing index, and the context afterwards
def test_lowest_invalid_index_across_workgroups(ctx, gold, big_bases):
    std, mont = big_bases
    n = 3000  # 12 workgroups of 256
    imgs = bytearray(mh.compress_points_g2(mont[:n], mh.FORM_MONT))
    bad = {e["name"]: bytes.fromhex(e["image_hex"]) for e in gold["invalid"]}
    plan = {2900: "both_flags", 1411: "order_10069", 777: "non_residue_x", 2048: "c1_ge_p", 1000: "random_twist_point"}
    for i, name in plan.items():
        imgs[64 * i:64 * i + 64] = bad[name]
    expect_invalid(lambda: ctx.decompress_g2(bytes(imgs), SUBGROUP), 777, "curve")
    expect_invalid(lambda: ctx.decompress_g2(bytes(imgs), 0), 777, "curve")  # (1000 and 1411 pass without the subgroup test)
    imgs[64 * 777:64 * 778] = mh.compress_points_g2(mont[777:778], mh.FORM_MONT)
    expect_invalid(lambda: ctx.decompress_g2(bytes(imgs), SUBGROUP), 1000, "subgroup")
    expect_invalid(lambda: ctx.decompress_g2(bytes(imgs), 0), 2048, "decode")
    xy, inf = ctx.decompress_g2(mh.compress_points_g2(mont[:n], mh.FORM_MONT), SUBGROUP)  # the context is still good
    assert (xy == mont[:n]).all() and not inf.any()


# 3. the root-and-sign routine on arbitrary Fq2 values
def test_hook_root_and_sign():
    rnd = random.Random(0xB254)
    vals, kind = [], []
    for _ in range(300):  # random squares
        t = (rnd.randrange(P), rnd.randrange(P))
        vals.append(g2.mul2(t, t)), kind.append("square")
    fq_res = fq_non = 0
    for _ in range(200):  # a = t in Fq: residues (roots with c1 = 0) and non-residues of Fq (roots with c0 = 0; alpha = a^((p-1)/2) = -1)
        t = rnd.randrange(1, P)
        res = pow(t, (P - 1) // 2, P) == 1
        fq_res, fq_non = fq_res + res, fq_non + (not res)
        vals.append((t, 0)), kind.append("fq")
    vals.append((0, 0)), kind.append("zero")
    vals += [(1, 0), (P - 1, 0), (0, 1), (0, P - 1), (4, 0), (P - 4, 0)]
    kind += ["fq"] * 6
    non = 0
    while non < 100:  # non-squares of Fq2
        t = (rnd.randrange(P), rnd.randrange(P))
        if g2.sqrt2(t) is None:
            vals.append(t), kind.append("nonsquare")
            non += 1
    a = np.array([g2.int_words(v[0]) + g2.int_words(v[1]) for v in vals], np.uint32)
    expect = [g2.sqrt2(v) for v in vals]
    # what the data must contain
    assert fq_res > 20 and fq_non > 20
    assert any(r is not None and r[1] == 0 and r[0] != 0 for r in expect), "no root with c1 = 0"
    assert any(r is not None and r[0] == 0 and r[1] != 0 for r in expect), "no root with c0 = 0"
    assert any(g2.pow2(v, (P - 1) // 2) == (P - 1, 0) for v in vals), "no input on the alpha = -1 branch"
    assert sum(r is None for r in expect) == 100
    with th.HooksContext() as c:
        for want in (0, 1):
            out, ok = c.test_g2_sqrt(a, np.full(len(vals), want, np.uint8))
            for i, (v, r) in enumerate(zip(vals, expect)):
                if r is None:
                    assert ok[i] == 0 and not out[i].any(), (kind[i], v)
                    continue
                assert ok[i] == 1, (kind[i], v)
                y = (g2.words_int(out[i][:8]), g2.words_int(out[i][8:]))
                assert y[0] < P and y[1] < P and g2.mul2(y, y) == v, (kind[i], v)
                assert y in (r, g2.neg2(r))
                if y != (0, 0):
                    assert g2.is_larger2(y) == bool(want), (kind[i], v, want)
        mixed = np.array([i & 1 for i in range(len(vals))], np.uint8)  # both requests inside one wavefront
        out, ok = c.test_g2_sqrt(a, mixed)
        for i, r in enumerate(expect):
            if r is not None and r != (0, 0):
                y = (g2.words_int(out[i][:8]), g2.words_int(out[i][8:]))
                assert g2.mul2(y, y) == vals[i] and g2.is_larger2(y) == bool(mixed[i])


# 4. round trip at size
@pytest.mark.parametrize("n", [1, 2, 255, 4096, 1 << 16, 1 << 20])
def test_round_trip_at_size(ctx, big_bases, n):
    std, mont = big_bases
    bases = tile(mont, n)
    imgs = mh.compress_points_g2(bases, mh.FORM_MONT)
    assert len(imgs) == 64 * n
    xy, inf = ctx.decompress_g2(imgs, SUBGROUP)
    assert (xy == bases).all() and not inf.any()
    mask = (np.arange(n) % 7 == 0).astype(np.uint8)  # every seventh point infinite
    imgs = mh.compress_points_g2(bases, mh.FORM_MONT, mask)
    xy, inf = ctx.decompress_g2(imgs, SUBGROUP)
    want = bases.copy()
    want[mask != 0] = 0
    assert (inf == mask).all() and (xy == want).all()


# 5. validation of uncompressed bases
def off_subgroup_point(gold):
    e = [e for e in gold["invalid"] if e["name"] == "random_twist_point"][0]
    m = mont_words(e["mont_le_hex"])
    v = g2.from_mont_words(m.tolist())
    return m, np.array(g2.point_words(((v[0], v[1]), (v[2], v[3]))), np.uint32)


def test_validate_g2_both_forms(ctx, big_bases, gold):
    std, mont = big_bases
    n = 5000
    for checks in (CURVE, SUBGROUP, CURVE | SUBGROUP):
        assert ctx.validate_g2(std[:n], mh.FORM_STD, checks=checks) is None
        assert ctx.validate_g2(mont[:n], mh.FORM_MONT, checks=checks) is None
    for form, base in ((mh.FORM_STD, std), (mh.FORM_MONT, mont)):
        b = base[:n].copy()
        b[1234, 16 + 3] ^= 0x10  # one word of y.c0 flipped
        for checks in (CURVE, SUBGROUP):
            expect_invalid(lambda: ctx.validate_g2(b, form, checks=checks), 1234, "curve")
        inf = np.zeros(n, np.uint8)
        inf[1234] = 1  # flagged infinite: passes whatever its coordinates
        assert ctx.validate_g2(b, form, inf, checks=CURVE | SUBGROUP) is None
    om, os_ = off_subgroup_point(gold)
    for form, base, off in ((mh.FORM_STD, std, os_), (mh.FORM_MONT, mont, om)):
        b = base[:n].copy()
        b[4321] = off
        assert ctx.validate_g2(b, form, checks=CURVE) is None
        expect_invalid(lambda: ctx.validate_g2(b, form, checks=SUBGROUP), 4321, "subgroup")
        expect_invalid(lambda: ctx.validate_g2(b, form, checks=CURVE | SUBGROUP), 4321, "subgroup")
        b[300, 8:16] = np.array(g2.int_words(P + 1), np.uint32)  # x.c1 >= p
        for checks in (CURVE, SUBGROUP):  # a coordinate out of range is the curve check's to refuse
            expect_invalid(lambda: ctx.validate_g2(b, form, checks=checks), 300, "curve")
    assert ctx.validate_g2(std[:n], mh.FORM_STD) is None  # the context is still good


def test_validate_g2_device_torch_stream(ctx, big_bases, gold):
    import torch
    std, mont = big_bases
    n = 20000
    dev = torch.device("cuda:0")
    om, _ = off_subgroup_point(gold)
    b = mont[:n].copy()
    db = torch.from_numpy(b.view(np.int32)).to(dev)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        assert ctx.validate_g2_device(db.data_ptr(), n, checks=SUBGROUP, stream=st.cuda_stream) is None
    assert ctx.validate_g2_device(db.data_ptr(), n, checks=CURVE) is None
    b[17000] = om
    b[19999, 24] ^= 1
    db2 = torch.from_numpy(b.view(np.int32)).to(dev)
    inf = np.zeros(n, np.uint8)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        expect_invalid(lambda: ctx.validate_g2_device(db2.data_ptr(), n, checks=SUBGROUP, stream=st.cuda_stream), 17000, "subgroup")
        expect_invalid(lambda: ctx.validate_g2_device(db2.data_ptr(), n, checks=CURVE, stream=st.cuda_stream), 19999, "curve")
        inf[17000] = inf[19999] = 1
        di = torch.from_numpy(inf).to(dev)
        st.synchronize()
        assert ctx.validate_g2_device(db2.data_ptr(), n, d_inf_ptr=di.data_ptr(), checks=SUBGROUP, stream=st.cuda_stream) is None
    # the host call agrees
    expect_invalid(lambda: ctx.validate_g2(b, mh.FORM_MONT, checks=SUBGROUP), 17000, "subgroup")


def test_validate_g1(ctx):
    for name in ("rand_n256", "rand_n17", "edge_inf_bases"):
        g = np.load(os.path.join(GOLDEN, f"msm_{name}.npz"))
        inf = g["inf"] if g["inf"].any() else None
        assert ctx.validate_g1(g["bases"], mh.FORM_STD, inf) is None
    g = np.load(os.path.join(GOLDEN, "msm_rand_n256.npz"))
    b = g["bases"].copy()
    b[200, 9] ^= 4
    expect_invalid(lambda: ctx.validate_g1(b, mh.FORM_STD), 200, "curve")
    inf = np.zeros(256, np.uint8)
    inf[200] = 1
    assert ctx.validate_g1(b, mh.FORM_STD, inf) is None
    xy, dinf = ctx.decompress(mh.compress_points(g["bases"], mh.FORM_STD))  # Montgomery words of the same points
    assert ctx.validate_g1(xy, mh.FORM_MONT) is None
    xy[5, 0] ^= 1
    expect_invalid(lambda: ctx.validate_g1(xy, mh.FORM_MONT), 5, "curve")
    b = g["bases"].copy()
    b[9, 0:8] = np.array(g2.int_words(P), np.uint32)  # x = p
    expect_invalid(lambda: ctx.validate_g1(b, mh.FORM_STD), 9, "curve")


# 6. end to end: images -> device buffers -> MSM
def test_decompress_device_then_msm(ctx, big_bases):
    import torch
    std, mont = big_bases
    n = 1 << 16
    rng = np.random.default_rng(66)
    s = rng.integers(0, 1 << 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)
    s[:, 7] &= 0x1FFFFFFF
    mask = (np.arange(n) % 11 == 5).astype(np.uint8)
    imgs = mh.compress_points_g2(mont[:n], mh.FORM_MONT, mask)
    dev = torch.device("cuda:0")
    d_xy = torch.empty(n * 32, dtype=torch.int32, device=dev)
    d_inf = torch.empty(n, dtype=torch.uint8, device=dev)
    ds = torch.from_numpy(s.view(np.int32)).to(dev)
    torch.cuda.synchronize()
    assert ctx.decompress_g2_device(imgs, d_xy.data_ptr(), d_inf.data_ptr(), SUBGROUP) == n
    r = ctx.msm_g2_device(d_xy.data_ptr(), ds.data_ptr(), n, d_inf_ptr=d_inf.data_ptr())
    ref = ctx.msm_g2(mont[:n], s, mh.FORM_MONT, mask)
    ints = [int.from_bytes(row.tobytes(), "little") for row in s]
    tot = sum(k * ((A0 + i * D0) % R) for i, k in enumerate(ints) if not mask[i]) % R
    exp = g2.mul(G, tot)
    assert not r.is_infinity and r.affine_std.tolist() == ref.affine_std.tolist() == g2.affine_words_std(exp)
    want = mont[:n].copy()
    want[mask != 0] = 0
    assert (d_xy.cpu().numpy().view(np.uint32).reshape(n, 32) == want).all() and (d_inf.cpu().numpy() == mask).all()
    st = torch.cuda.Stream(device=dev)  # on a caller's stream, without the subgroup test
    d_xy.zero_()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        ctx.decompress_g2_device(imgs, d_xy.data_ptr(), d_inf.data_ptr(), 0, stream=st.cuda_stream)
    assert (d_xy.cpu().numpy().view(np.uint32).reshape(n, 32) == want).all()


# 7. argument errors
def test_error_paths(ctx, big_bases):
    std, mont = big_bases
    for checks in (0, 4, 7, 1 << 31):
        with pytest.raises(mh.MsmError) as e:
            ctx.validate_g2(std[:4], mh.FORM_STD, checks=checks)
        assert e.value.code == mh.ERR_BAD_ARG
    with pytest.raises(mh.MsmError) as e:
        ctx.validate_g2(std[:4], 5)
    assert e.value.code == mh.ERR_BAD_ARG
    with pytest.raises(mh.MsmError) as e:
        ctx.decompress_g2(mh.compress_points_g2(std[:4]), 4)
    assert e.value.code == mh.ERR_BAD_ARG
    lib, h = ctx._lib, ctx._h
    assert lib.msm_bn254_g2_validate(h, mh._p32(std), mh.FORM_STD, None, 0, SUBGROUP, None) == mh.ERR_EMPTY
    assert lib.msm_bn254_g1_validate(h, mh._p32(std), mh.FORM_STD, None, 0, None) == mh.ERR_EMPTY
    assert lib.msm_bn254_g2_validate_device(h, 4096, None, 0, SUBGROUP, None, None) == mh.ERR_EMPTY
    assert lib.msm_bn254_g2_validate_device(h, 4096, None, 4, 0, None, None) == mh.ERR_BAD_ARG
    assert lib.msm_bn254_g2_decompress(h, None, 0, 0, None, None, None) == mh.ERR_EMPTY
    assert lib.msm_bn254_g2_decompress_device(h, None, 0, 0, None, None, None, None) == mh.ERR_EMPTY
    assert lib.msm_bn254_g2_validate(h, None, mh.FORM_STD, None, 4, SUBGROUP, None) == mh.ERR_BAD_ARG
    for call in (lambda: ctx.decompress_g2(b""), lambda: ctx.validate_g2(np.zeros((0, 32), np.uint32)), lambda: ctx.validate_g1(np.zeros((0, 16), np.uint32)),
                 lambda: ctx.validate_g2_device(4096, 0)):
        with pytest.raises(mh.MsmError) as e:
            call()
        assert e.value.code == mh.ERR_EMPTY
    with pytest.raises(mh.MsmError) as e:
        ctx.decompress_g2(bytes(65))
    assert e.value.code == mh.ERR_BAD_ARG
    assert ctx.validate_g2(std[:4], mh.FORM_STD) is None  # still usable
