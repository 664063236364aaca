"""The G1 element-wise multiplication on the GPU (-m gpu): msm_bn254_g1_pointwise_mul(_device) and msm_bn254_g1_scale_device against the CPU
oracle -- sizes around the inversion group under every flag, the edge scalars of the split and the ladder, identities at every place of a group,
one scalar for all points, in place, the points of a real proving key, errors, two streams, the host form, and the two ceremony updates (a
powers-of-tau contribution, a phase-2 contribution) end to end on one stream.  Inputs come from fixed seeds; every comparison is word-exact."""
import os
import sys

import numpy as np
import pytest

import mopro_msm_hip as mh
from oracle import bn254_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pointwise_mul_cases as pm  # noqa: E402

pytestmark = pytest.mark.gpu
P, R = pm.P, pm.R
IM, OS, BS = mh.NTT_IN_MONT, mh.FB_OUT_STD, getattr(mh, "PM_BASES_STD", 16)
FILL = 0x5A  # every byte of the outputs before a call: a record the kernel skips shows up
G = 256      # the inversion group; test_sizes... checks it against the plan
SIZES = sorted({1, 2, 63, 64, 65, G - 1, G, G + 1, 2 * G + 1, 4096})
NMAX = 4096


@pytest.fixture(scope="module")
def ctx():
    c = mh.MsmContext()
    yield c
    c.close()


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32 if a.dtype == np.uint32 else np.uint8).copy()).to("cuda:0")


def outputs(n):
    return dev(np.full((n, 16), FILL * 0x01010101, np.uint32)), dev(np.full(n, FILL, np.uint8))


def host(d_xy, d_inf):
    import torch
    torch.cuda.synchronize()
    return d_xy.cpu().numpy().view(np.uint32).reshape(-1, 16), d_inf.cpu().numpy().view(np.uint8)


def device_mul(c, base_words, k_words, inf=None, flags=0, stream=None):
    import torch
    n = k_words.shape[0]
    d_b, d_k = dev(base_words), dev(k_words)
    d_m = None if inf is None else dev(np.asarray(inf, np.uint8))
    d_xy, d_inf = outputs(n)
    torch.cuda.synchronize()  # the arrays were made on torch's stream
    c.pointwise_mul_device(d_b.data_ptr(), d_k.data_ptr(), n, d_xy.data_ptr(), d_inf.data_ptr(), None if d_m is None else d_m.data_ptr(), flags, stream)
    return host(d_xy, d_inf)


def device_scale(c, base_words, k, inf=None, flags=0, stream=None):
    import torch
    n = base_words.shape[0]
    d_b = dev(base_words)
    d_m = None if inf is None else dev(np.asarray(inf, np.uint8))
    d_xy, d_inf = outputs(n)
    torch.cuda.synchronize()
    c.scale_device(d_b.data_ptr(), k, n, d_xy.data_ptr(), d_inf.data_ptr(), None if d_m is None else d_m.data_ptr(), flags, stream)
    return host(d_xy, d_inf)


def same(got, want, what=None):
    (xy, inf), (wxy, winf) = got, want
    assert xy.shape == wxy.shape and inf.shape == winf.shape, what
    bad = np.flatnonzero((xy != wxy).any(axis=1) | (inf != winf))
    assert bad.size == 0, (what, "first wrong point", int(bad[0]), "of", xy.shape[0], "wrong", int(bad.size))


def cut(want, n):
    return want[0][:n], want[1][:n]


@pytest.fixture(scope="module")
def ref():
    """4096 seeded bases b_i * G in both forms, 4096 seeded 256-bit patterns, and what the call must give for them per flag set, computed once;
    the tests take prefixes and leave it unchanged"""
    ks, bs = pm.patterns(0x9017F1, NMAX), pm.logs(0x9017F2, NMAX)
    inv_mont = pow(pm.MONT_R, -1, R)
    mont = pm.expected(ks, bs)
    return {"ks": ks, "bs": bs, "k_words": pm.to_words(ks), "mont": pm.bases(bs, pm.FORM_MONT), "std": pm.bases(bs, pm.FORM_STD),
            "want": {0: mont, OS: pm.expected(ks, bs, out_std=True), IM: pm.expected([k * inv_mont % R for k in ks], bs), BS: mont}}


# 1
@pytest.mark.parametrize("flags", [0, OS, IM, BS])
@pytest.mark.parametrize("n", SIZES)
def test_sizes_around_the_inversion_group(ctx, ref, n, flags):
    assert mh.pointwise_mul_plan()["inv_group"] == G
    got = device_mul(ctx, ref["std" if flags & BS else "mont"][:n], ref["k_words"][:n], flags=flags)
    same(got, cut(ref["want"][flags], n), (n, flags))


# 2
def test_edge_scalars_on_three_bases(ctx):
    ks = pm.edge_scalars()
    assert ks[:9] == [0, 1, 2, 3, R - 1, R, R + 1, 2 * R, 5 * R] and ks[11] == pm.LAMBDA
    for b in (1, 0xC0FFEE, R - 2):
        bs = [b] * len(ks)
        std = pm.bases(bs, pm.FORM_STD)
        got = device_mul(ctx, std, pm.to_words(ks), flags=OS | BS)
        same(got, pm.expected(ks, bs, out_std=True), b)
        xy, inf = got
        x, y = pm.point_ints(std[0])
        assert list(inf[:9]) == [1, 0, 0, 0, 0, 1, 0, 1, 1]
        assert (xy[1] == std[0]).all() and (xy[6] == std[0]).all()                   # 1 * P and (r + 1) * P return P's words
        assert pm.point_ints(xy[4]) == (x, P - y)                                     # (r - 1) * P = -P: same x, y = p - y
        assert pm.point_ints(xy[11]) == (pm.BETA * x % P, y)                          # lambda * P = (beta x, y)
        mont = pm.bases(bs[:12], pm.FORM_MONT)
        got = device_mul(ctx, mont, pm.to_words(ks[:12]))
        assert (got[0][1] == mont[0]).all() and not got[0][0].any() and got[1][0] == 1  # the same in Montgomery words


# 3
def test_identities_at_every_place_of_a_group(ctx, ref):
    n = 2 * G + 1
    zeros = [0, R, 2 * R, 5 * R]
    places = {"first of a group": [0, G, 2 * G], "last of a group": [G - 1, 2 * G - 1], "a whole group": list(range(G, 2 * G)),
              "every second lane": list(range(0, n, 2)), "all": list(range(n))}
    want = cut(ref["want"][0], n)
    for name, at in places.items():
        hit = np.zeros(n, bool)
        hit[at] = True
        mixed = list(ref["ks"][:n])
        for t, i in enumerate(at):
            mixed[i] = zeros[t % 4]
        flagged = ref["mont"][:n].copy()
        flagged[hit] = 0xDEADBEEF  # the words of a flagged base are not read as a point
        for how, got in (("scalars = 0 mod r", device_mul(ctx, ref["mont"][:n], pm.to_words(mixed))),
                         ("flagged bases", device_mul(ctx, flagged, ref["k_words"][:n], inf=hit.astype(np.uint8)))):
            xy, inf = got
            assert (inf[hit] == 1).all() and not xy[hit].any(), (name, how)                    # flagged, coordinates all zero
            assert (inf[~hit] == 0).all() and (xy[~hit] == want[0][~hit]).all(), (name, how)  # every neighbour still exact


# 4
def test_one_scalar_for_all_points(ctx, ref):
    import torch
    n = 2 * G + 1
    inf = np.zeros(n, np.uint8)
    inf[[0, G - 1, G]] = 1
    for k in (0, 1, R - 1, pm.LAMBDA, pm.patterns(0x5CA1E, 1)[0] | 1 << 255):
        assert k < R or k >> 255
        want = pm.expected([k] * n, ref["bs"][:n], inf)
        got = device_scale(ctx, ref["mont"][:n], k, inf)
        same(got, want, ("scale against the oracle", hex(k)))
        same(got, device_mul(ctx, ref["mont"][:n], pm.to_words([k] * n), inf), ("scale against the per-element call", hex(k)))
    same(device_scale(ctx, ref["std"][:n], 5, flags=OS | BS), pm.expected([5] * n, ref["bs"][:n], out_std=True), "standard form in and out")
    d_b = dev(ref["mont"][:4])
    d_xy, d_inf = outputs(4)
    torch.cuda.synchronize()
    with pytest.raises(mh.MsmError) as e:
        ctx.scale_device(d_b.data_ptr(), 5, 4, d_xy.data_ptr(), d_inf.data_ptr(), flags=IM)
    assert e.value.code == mh.ERR_BAD_ARG
    got = host(d_xy, d_inf)
    assert (got[0] == FILL * 0x01010101).all() and (got[1] == FILL).all()


# 5
def test_in_place(ctx, ref):
    import torch
    n = 2 * G + 1
    inf = np.zeros(n, np.uint8)
    inf[[3, G, n - 1]] = 1
    want = pm.expected(ref["ks"][:n], ref["bs"][:n], inf)
    same(device_mul(ctx, ref["mont"][:n], ref["k_words"][:n], inf), want, "out of place")
    d_b, d_k, d_m = dev(ref["mont"][:n]), dev(ref["k_words"][:n]), dev(inf)
    torch.cuda.synchronize()
    ctx.pointwise_mul_device(d_b.data_ptr(), d_k.data_ptr(), n, d_b.data_ptr(), d_m.data_ptr(), d_m.data_ptr())
    same(host(d_b, d_m), want, "in place")
    d_b, d_m = dev(ref["mont"][:n]), dev(inf)
    torch.cuda.synchronize()
    ctx.scale_device(d_b.data_ptr(), 7, n, d_b.data_ptr(), d_m.data_ptr(), d_m.data_ptr())
    same(host(d_b, d_m), pm.expected([7] * n, ref["bs"][:n], inf), "one scalar, in place")


# 6
def test_points_of_a_proving_key():
    """bases that are no known multiple of the generator: the G1 entries of tests/golden/zkey_g1_points.json, expected values per point from
    the oracle's scalar multiplication"""
    from conftest import load_zkey_points
    bases, inf, _, _, _ = load_zkey_points()
    n = bases.shape[0]
    assert n == 19
    ks = pm.patterns(0x2CE7, n)
    ks[2], ks[5] = 0, R
    wxy, winf = np.zeros((n, 16), np.uint32), np.zeros(n, np.uint8)
    for i in range(n):
        if inf[i]:
            winf[i] = 1
            continue
        std = np.concatenate([orc.fq_from_mont(bases[i, :8]), orc.fq_from_mont(bases[i, 8:])])
        wxy[i], winf[i] = orc.g1_to_affine_std(orc.g1_scalar_mul(std, pm.words(ks[i] % R)))
    assert winf[2] == 1 and winf[5] == 1 and winf.sum() < n - 8
    with mh.MsmContext() as c:
        same(device_mul(c, bases, pm.to_words(ks), inf, flags=OS), (wxy, winf), "zkey points")
        same(c.pointwise_mul(bases, pm.to_words(ks), mh.FORM_MONT, inf, flags=OS), (wxy, winf), "zkey points, host form")


# 7
def test_errors_write_nothing(ctx, ref):
    import torch
    n = 70
    lib = mh.load_library()
    d_b, d_k, d_m = dev(ref["mont"][:n + 1]), dev(ref["k_words"][:n + 1]), dev(np.zeros(n + 16, np.uint8))
    d_xy, d_inf = outputs(n + 16)
    torch.cuda.synchronize()
    b, k, m, xy, inf = (t.data_ptr() for t in (d_b, d_k, d_m, d_xy, d_inf))
    bad = [((None, k, n, xy, inf), {}), ((b, None, n, xy, inf), {}), ((b, k, n, None, inf), {}), ((b, k, n, xy, None), {}),
           ((b + 4, k, n, xy, inf), {}), ((b, k + 8, n, xy, inf), {}), ((b, k, n, xy + 4, inf), {}), ((b, k, n, xy, inf + 1), {}),
           ((b, k, n, xy, inf), {"d_inf": m + 1}), ((b, k, n, xy, inf), {"flags": 1}), ((b, k, n, xy, inf), {"flags": 4}), ((b, k, n, xy, inf), {"flags": 32})]
    for args, kw in bad:
        with pytest.raises(mh.MsmError) as e:
            ctx.pointwise_mul_device(*args, **kw)
        assert e.value.code == mh.ERR_BAD_ARG, (args, kw)
        if args[1] is not None and args[1] == k:  # the same pointers and flags through the one-scalar call
            with pytest.raises(mh.MsmError) as e:
                ctx.scale_device(args[0], 3, *args[2:], **kw)
            assert e.value.code == mh.ERR_BAD_ARG, (args, kw)
    assert lib.msm_bn254_g1_scale_device(ctx._h, b, None, None, n, 0, xy, inf, None) == mh.ERR_BAD_ARG  # no scalar
    for call in (lambda: ctx.pointwise_mul_device(b, k, 0, xy, inf), lambda: ctx.scale_device(b, 3, 0, xy, inf),
                 lambda: ctx.pointwise_mul(np.zeros((0, 16), np.uint32), np.zeros((0, 8), np.uint32))):
        with pytest.raises(mh.MsmError) as e:
            call()
        assert e.value.code == mh.ERR_EMPTY
    h_xy, h_inf = np.full((n, 16), FILL * 0x01010101, np.uint32), np.full(n, FILL, np.uint8)
    hb, hk = np.ascontiguousarray(ref["mont"][:n]), np.ascontiguousarray(ref["k_words"][:n])
    p32, p8 = lambda a: a.ctypes.data_as(mh._u32p), lambda a: a.ctypes.data_as(mh._u8p)
    for form, flags in ((2, 0), (mh.FORM_MONT, 1), (mh.FORM_MONT, BS), (mh.FORM_MONT, 64)):
        assert lib.msm_bn254_g1_pointwise_mul(ctx._h, p32(hb), form, None, p32(hk), n, flags, p32(h_xy), p8(h_inf)) == mh.ERR_BAD_ARG, (form, flags)
    for args in ((None, p32(hk), p32(h_xy), p8(h_inf)), (p32(hb), None, p32(h_xy), p8(h_inf)), (p32(hb), p32(hk), None, p8(h_inf)),
                 (p32(hb), p32(hk), p32(h_xy), None)):
        assert lib.msm_bn254_g1_pointwise_mul(ctx._h, args[0], mh.FORM_MONT, None, args[1], n, 0, args[2], args[3]) == mh.ERR_BAD_ARG
    got = host(d_xy, d_inf)
    assert (got[0] == FILL * 0x01010101).all() and (got[1] == FILL).all()          # no failed call wrote anything
    assert (h_xy == FILL * 0x01010101).all() and (h_inf == FILL).all()
    same(device_mul(ctx, ref["mont"][:n], ref["k_words"][:n]), cut(ref["want"][0], n), "a correct call after the errors")


# 8
def test_two_streams(ctx, ref):
    import torch
    n, m = 2 * G + 1, 1000
    d_b1, d_k1, d_b2 = dev(ref["mont"][:n]), dev(ref["k_words"][:n]), dev(ref["std"][n:n + m])
    xy1, inf1 = outputs(n)
    xy2, inf2 = outputs(m)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    ctx.pointwise_mul_device(d_b1.data_ptr(), d_k1.data_ptr(), n, xy1.data_ptr(), inf1.data_ptr(), stream=s1.cuda_stream)
    ctx.scale_device(d_b2.data_ptr(), R - 3, m, xy2.data_ptr(), inf2.data_ptr(), flags=OS | BS, stream=s2.cuda_stream)
    same(host(xy1, inf1), cut(ref["want"][0], n), "stream 1")
    same(host(xy2, inf2), pm.expected([R - 3] * m, ref["bs"][n:n + m], out_std=True), "stream 2")


# 9
def test_host_pointer_form_equals_device_form(ctx, ref):
    n = 2 * G + 1
    inf = np.zeros(n, np.uint8)
    inf[[0, G]] = 1
    for form, key in ((mh.FORM_MONT, "mont"), (mh.FORM_STD, "std")):
        for flags in (0, OS):
            xy, out_inf = ctx.pointwise_mul(ref[key][:n], ref["k_words"][:n], form, inf, flags)
            same((xy, out_inf), device_mul(ctx, ref[key][:n], ref["k_words"][:n], inf, flags | (BS if form == mh.FORM_STD else 0)), (form, flags))
            same((xy, out_inf), pm.expected(ref["ks"][:n], ref["bs"][:n], inf, bool(flags & OS)), (form, flags))
    same(ctx.pointwise_mul(ref["mont"][:n], ref["k_words"][:n], mh.FORM_MONT), cut(ref["want"][0], n), "no mask")


# 10
def test_powers_of_tau_contribution_in_hbm(ctx):
    """tauG1[i] = tau^i * G made in HBM, then updated in place by tau'^i -- one non-default stream, nothing crossing PCIe in between -- is word
    for word the array made from the powers of tau * tau'; it then serves msm_bn254_g1_device as its bases"""
    import torch
    n = 1025
    tau, tau2 = pm.patterns(0x7A0, 2)
    tau, tau2 = tau % R, tau2 % R
    gen = np.concatenate([pm.words(1), pm.words(2)])
    s = orc.gen_scalars(0xB2540014, n)
    d_s = dev(s)
    d_k, d_k2, d_kk = (dev(np.zeros((n, 8), np.uint32)) for _ in range(3))
    d_xy, d_inf = outputs(n)
    w_xy, w_inf = outputs(n)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    q = st.cuda_stream
    ctx.fr_powers_device(tau, d_k.data_ptr(), n, stream=q)
    ctx.fixed_base_mul_device(gen, d_k.data_ptr(), n, d_xy.data_ptr(), d_inf.data_ptr(), stream=q)
    ctx.fr_powers_device(tau2, d_k2.data_ptr(), n, stream=q)
    ctx.pointwise_mul_device(d_xy.data_ptr(), d_k2.data_ptr(), n, d_xy.data_ptr(), d_inf.data_ptr(), d_inf.data_ptr(), stream=q)
    r = ctx.msm_device(d_xy.data_ptr(), d_s.data_ptr(), n, d_inf.data_ptr(), stream=q)
    ctx.fr_powers_device(tau * tau2 % R, d_kk.data_ptr(), n, stream=q)
    ctx.fixed_base_mul_device(gen, d_kk.data_ptr(), n, w_xy.data_ptr(), w_inf.data_ptr(), stream=q)
    got = host(d_xy, d_inf)
    same(got, host(w_xy, w_inf), "against the fixed-base call on (tau tau')^i")
    logs = [pow(tau * tau2 % R, i, R) for i in range(n)]
    same(cut(got, 40), pm.expected([1] * 40, logs[:40]), "a prefix against the oracle")
    want, winf = orc.closed_form_expected(pm.to_words(logs), s)
    assert not winf and not r.is_infinity and (r.affine_std == want).all()


# 11
def test_phase2_contribution(ctx, ref):
    """every point times 1 / delta', and back with delta'"""
    import torch
    n = 2 * G + 1
    delta = pm.patterns(0xDE17A, 1)[0] % R
    inv = pow(delta, -1, R)
    d_b = dev(ref["mont"][:n])
    d_xy, d_inf = outputs(n)
    b_xy, b_inf = outputs(n)
    torch.cuda.synchronize()
    ctx.scale_device(d_b.data_ptr(), inv, n, d_xy.data_ptr(), d_inf.data_ptr())
    ctx.scale_device(d_xy.data_ptr(), delta, n, b_xy.data_ptr(), b_inf.data_ptr(), d_inf.data_ptr())
    same(host(d_xy, d_inf), pm.expected([inv] * n, ref["bs"][:n]), "times 1 / delta'")
    same(host(b_xy, b_inf), (ref["mont"][:n], np.zeros(n, np.uint8)), "and back")


# 12
def test_the_staging_boundary_on_both_forms(ctx, ref):
    """2^20 + 513 points: the host-pointer form stages 2^20 at a time, so its loop runs twice, with one flagged base in each step"""
    n = (1 << 20) + 513
    reps = -(-n // 513)
    bases = np.tile(ref["mont"][:513], (reps, 1))[:n]
    words = np.tile(ref["k_words"][:513], (reps, 1))[:n]
    want = (np.tile(ref["want"][0][0][:513], (reps, 1))[:n], np.tile(ref["want"][0][1][:513], reps)[:n])
    inf = np.zeros(n, np.uint8)
    for at in (5, (1 << 20) + 7):  # neither is an identity of the expectation already
        assert want[1][at] == 0
        inf[at], want[0][at], want[1][at] = 1, 0, 1
    same(ctx.pointwise_mul(bases, words, mh.FORM_MONT, inf), want, "host form")
    same(device_mul(ctx, bases, words, inf), want, "device form")
