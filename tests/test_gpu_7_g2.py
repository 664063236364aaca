"""BN254 G2 MSM on the GPU (-m gpu): msm_bn254_g2 / msm_bn254_g2_device against the independent Python law (tools/bn254_g2_py.py).

Large instances use bases P_i = (a + (i mod M) * d) * G2, built once per session from M additions of d * G2 (batched affine additions, one field
inversion per batch), so the answer is a single scalar multiplication: (sum_i s_i (a + (i mod M) d) mod r) * G2."""
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

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden")
P, R, G = g2.P, g2.R, g2.G2_GEN
M = 1 << 18  # distinct bases of the large instances
A0, D0 = 0x1234567890ABCDEF1234567890ABCDEF, 0xFEDCBA987654321


@pytest.fixture(scope="session")
def big_bases():
    """M x 32 Montgomery words of P_i = (A0 + i * D0) * G2, and the same in standard form"""
    pts = g2.chain_points(A0, D0, M)
    std = np.array([g2.point_words(p_) for p_ in pts[:M]], np.uint32)
    to_m = lambda v: v * g2.R256 % P
    mont = np.array([[w for c in (p_[0][0], p_[0][1], p_[1][0], p_[1][1]) for w in g2.int_words(to_m(c))] for p_ in pts[:M]], np.uint32)
    return std, mont


def coeffs(n):
    return [(A0 + (i % M) * D0) % R for i in range(n)]


def expected(scalars_words, n, inf=None):
    ints = [int.from_bytes(r.tobytes(), "little") for r in np.ascontiguousarray(scalars_words[:n], np.uint32)]
    c = coeffs(n)
    tot = sum(s * k for i, (s, k) in enumerate(zip(ints, c)) if inf is None or not inf[i]) % R
    return g2.mul(G, tot)


def tile(arr, n):
    reps = (n + M - 1) // M
    return np.ascontiguousarray(np.tile(arr, (reps, 1))[:n])


def rand_scalars(seed, n, bits=253):
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 1 << 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)
    if bits < 256:
        for w in range(8):
            lo = 32 * w
            if lo >= bits:
                s[:, w] = 0
            elif bits - lo < 32:
                s[:, w] &= np.uint32((1 << (bits - lo)) - 1)
    return s


def check(r, exp):
    assert r.is_infinity == (exp is None)
    assert r.affine_std.tolist() == g2.affine_words_std(exp)


@pytest.fixture(scope="module")
def ctx():
    c = mh.MsmContext()
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_noglv():
    c = mh.MsmContext(flags=mh.FLAG_NO_GLV)
    yield c
    c.close()


def g2_vectors():
    with open(os.path.join(GOLDEN, "g2_index.json")) as f:
        return [v["file"] for v in json.load(f)["vectors"]]


# 1. goldens, both forms
@pytest.mark.parametrize("fn", g2_vectors())
def test_g2_goldens_both_forms(ctx, fn):
    g = np.load(os.path.join(GOLDEN, fn))
    inf = g["inf"] if g["inf"].any() else None
    for form, key in ((mh.FORM_STD, "bases"), (mh.FORM_MONT, "bases_mont")):
        r = ctx.msm_g2(g[key], g["scalars"], form, inf)
        assert r.is_infinity == bool(g["expected_inf"])
        assert (r.affine_std == g["expected"]).all(), (fn, form)


# 2. the zkey's G2 points with seeded scalars
def test_g2_zkey_points(ctx):
    with open(os.path.join(GOLDEN, "zkey_g2_points.json")) as f:
        pts = json.load(f)["points"]
    words = np.stack([np.frombuffer(bytes.fromhex(p_["mont_le_hex"]), "<u4") for p_ in pts]).astype(np.uint32)
    inf = np.array([p_["infinity"] for p_ in pts], np.uint8)
    ri = pow(g2.R256, -1, P)
    aff = [None if p_["infinity"] else tuple((g2.words_int(w[8 * c:8 * c + 8]) * ri % P, g2.words_int(w[8 * c + 8:8 * c + 16]) * ri % P)
                                              for c in (0, 2)) for p_, w in zip(pts, words)]
    rnd = random.Random(0xB25B2)
    for trial in range(3):
        sc = [rnd.randrange(R) for _ in pts]
        if trial == 1:
            sc[0], sc[-1] = R - 1, 1
        exp = g2.msm([a for a in aff if a is not None], [s for s, a in zip(sc, aff) if a is not None])
        r = ctx.msm_g2(words, np.array([g2.int_words(s) for s in sc], np.uint32), mh.FORM_MONT, inf)
        check(r, exp)
        b2 = [i for i, p_ in enumerate(pts) if p_["section"] == "B2"]  # the B query alone (3 of its 4 points at infinity)
        exp_b = g2.msm([aff[i] for i in b2 if aff[i] is not None], [sc[i] for i in b2 if aff[i] is not None])
        check(ctx.msm_g2(words[b2], np.array([g2.int_words(sc[i]) for i in b2], np.uint32), mh.FORM_MONT, inf[b2]), exp_b)


# 3. sizes, GLV on and off
@pytest.mark.parametrize("n", [1, 2, 3, 17, 255, 256, 1024, 4096, 1 << 16])
def test_g2_sizes(ctx, ctx_noglv, big_bases, n):
    std, mont = big_bases
    s = rand_scalars(n, n)
    exp = expected(s, n)
    check(ctx.msm_g2(std[:n], s, mh.FORM_STD), exp)
    check(ctx_noglv.msm_g2(mont[:n], s, mh.FORM_MONT), exp)


# 4. window widths and unsigned digits
@pytest.mark.parametrize("wb,flags", [(11, 0), (13, 0), (0, mh.FLAG_UNSIGNED_DIGITS), (13, mh.FLAG_UNSIGNED_DIGITS | mh.FLAG_NO_GLV)])
def test_g2_window_and_digit_configs(big_bases, wb, flags):
    std, mont = big_bases
    n = 4096
    s = rand_scalars(wb * 7 + flags, n)
    with mh.MsmContext(window_bits=wb, flags=flags) as c:
        check(c.msm_g2(mont[:n], s, mh.FORM_MONT), expected(s, n))


# 5. skewed scalars: the mid and long combine lists
def skewed(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "all_equal":
        return np.tile(rand_scalars(seed, 1), (n, 1))
    if kind in ("two", "three", "d256"):
        k = {"two": 2, "three": 3, "d256": 256}[kind]
        vals = rand_scalars(seed, k)
        return np.ascontiguousarray(vals[rng.integers(0, k, n)])
    if kind == "lt2p32":
        return rand_scalars(seed, n, bits=32)
    if kind == "fixture_t128":  # one sequence repeated T = 128 times
        return np.ascontiguousarray(np.tile(rand_scalars(seed, n // 128), (128, 1)))
    raise ValueError(kind)


@pytest.mark.parametrize("n", [1 << 16, 1 << 18])
@pytest.mark.parametrize("kind", ["all_equal", "two", "three", "d256", "lt2p32", "fixture_t128"])
def test_g2_skewed(ctx, big_bases, n, kind):
    std, mont = big_bases
    s = skewed(kind, n, n + len(kind))
    check(ctx.msm_g2(mont[:n], s, mh.FORM_MONT), expected(s, n))


# 6. infinity mask, all-zero scalars
def test_g2_infinity_mask_and_zero_scalars(ctx, big_bases):
    std, mont = big_bases
    n = 5000
    s = rand_scalars(6, n)
    inf = (np.arange(n) % 7 == 3).astype(np.uint8)
    check(ctx.msm_g2(std[:n], s, mh.FORM_STD, inf), expected(s, n, inf))
    r = ctx.msm_g2(std[:n], np.zeros((n, 8), np.uint32), mh.FORM_STD)
    assert r.is_infinity and not r.affine_std.any()
    check(ctx.msm_g2(std[:n], s, mh.FORM_STD, np.ones(n, np.uint8)), None)


# 7. a scalar >= 2^254 fails the call, the context stays usable
def test_g2_bad_scalar_then_good_call(ctx, big_bases):
    std, mont = big_bases
    n = 300
    s = rand_scalars(7, n)
    bad = s.copy()
    bad[17, 7] = 0xFFFFFFFF
    with pytest.raises(mh.MsmError) as e:
        ctx.msm_g2(std[:n], bad, mh.FORM_STD)
    assert e.value.code == mh.ERR_BAD_ARG
    check(ctx.msm_g2(std[:n], s, mh.FORM_STD), expected(s, n))
    with pytest.raises(mh.MsmError) as e:
        ctx.msm_g2(std[:n], s, 7)
    assert e.value.code == mh.ERR_BAD_ARG


# 8. the device entry, torch tensors on a non-default stream
def test_g2_device_entry_torch_stream(ctx, big_bases):
    import torch
    std, mont = big_bases
    n = 20000
    s = rand_scalars(8, n)
    inf = (np.arange(n) % 11 == 0).astype(np.uint8)
    dev = torch.device("cuda:0")
    db = torch.from_numpy(mont[:n].view(np.int32)).to(dev)
    ds = torch.from_numpy(s.view(np.int32)).to(dev)
    di = torch.from_numpy(inf).to(dev)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        r = ctx.msm_g2_device(db.data_ptr(), ds.data_ptr(), n, d_inf_ptr=di.data_ptr(), stream=st.cuda_stream)
    check(r, expected(s, n, inf))
    r = ctx.msm_g2_device(db.data_ptr(), ds.data_ptr(), n)
    check(r, expected(s, n))
    t = ctx.timings()
    assert t["num_points"] == n and t["num_adds"] > 0


# 9. full sizes
@pytest.mark.parametrize("n,glv", [(1 << 20, True), (1 << 20, False), (1 << 22, True)])
def test_g2_full_sizes(ctx, ctx_noglv, big_bases, n, glv):
    std, mont = big_bases
    s = rand_scalars(n + glv, n)
    c = ctx if glv else ctx_noglv
    check(c.msm_g2(tile(mont, n), s, mh.FORM_MONT), expected(s, n))


# 10. MSM_FLAG_DETERMINISTIC: the same 48 words every call
def test_g2_deterministic_words(big_bases):
    std, mont = big_bases
    n = 1 << 14
    s = skewed("d256", n, 10)
    exp = expected(s, n)
    with mh.MsmContext(flags=mh.FLAG_DETERMINISTIC) as c:
        outs = [c.msm_g2(mont[:n], s, mh.FORM_MONT).jacobian_mont.tolist() for _ in range(4)]
    assert all(o == outs[0] for o in outs)
    assert outs[0] == g2.jacobian_mont_words(exp)


# 11. G1 and G2 calls interleaved on the same contexts (shared flag words and call numbers), and fresh contexts
def test_g1_g2_interleaved_known_answers():
    with open(os.path.join(GOLDEN, "index.json")) as f:
        g1_cases = [c["name"] for c in json.load(f)["cases"]]
    g1v = [np.load(os.path.join(GOLDEN, f"msm_{c}.npz")) for c in g1_cases if c in ("rand_n17", "rand_n256", "rand_n3", "edge_p_minus_p")]
    g2v = [np.load(os.path.join(GOLDEN, f"msm_g2_{c}.npz")) for c in ("rand_n17", "rand_n256", "rand_n3", "edge_p_minus_p", "edge_inf_bases")]
    rnd = random.Random(11)
    ctxs = [mh.MsmContext(), mh.MsmContext(flags=mh.FLAG_NO_GLV)]
    bad = 0
    try:
        for i in range(2000):
            c = ctxs[i % 2]
            if rnd.random() < 0.5:
                g = rnd.choice(g1v)
                r = c.msm(g["bases"], g["scalars"], mh.FORM_STD, g["inf"] if g["inf"].any() else None)
            else:
                g = rnd.choice(g2v)
                r = c.msm_g2(g["bases_mont"], g["scalars"], mh.FORM_MONT, g["inf"] if g["inf"].any() else None)
            bad += int(not (r.affine_std == g["expected"]).all())
            if i % 500 == 499:
                with mh.MsmContext() as fresh:
                    g = g2v[0]
                    bad += int(not (fresh.msm_g2(g["bases"], g["scalars"]).affine_std == g["expected"]).all())
    finally:
        for c in ctxs:
            c.close()
    assert bad == 0
