"""The G1 group transform on the GPU (-m gpu): msm_bn254_g1_fft(_device) against the closed form of tools/g1_fft_cases.py -- the points of the Fr
transform of the inputs' logarithms -- at sizes below a wavefront, below, at and above a workgroup of butterflies, under every flag, in batches,
on the halo2 KZG parameter sets the reference ships, on the structured vectors whose butterflies double, cancel and meet the identity, there and
back, as the step from powers of tau to the Lagrange basis on one stream, after every error, on two streams and through the host form.  Inputs
come from fixed seeds; every comparison is word-exact."""
import os
import sys

import numpy as np
import pytest

import mopro_msm_hip as mh
from oracle import bn254_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import g1_fft_cases as gc  # noqa: E402

pytestmark = pytest.mark.gpu
P, R = gc.P, gc.R
INV, OS, BS = gc.INVERSE, gc.OUT_STD, gc.IN_STD
FILL = 0x5A  # every byte of an output before a call: a record the kernel skips, or one it must not touch, shows up
LOG_NS = [0, 1, 2, 3, 7, 8, 9, 10, 12]  # butterflies: none, 1 .. 4 (below a wavefront), 64, 128 (below a workgroup), 256 (one), 512 (two), 2048


@pytest.fixture(scope="module")
def ctx():
    c = mh.MsmContext()
    yield c
    c.close()


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32 if a.dtype == np.uint32 else np.uint8).copy()).to("cuda:0")


def host(d_xy, d_inf):
    import torch
    torch.cuda.synchronize()
    return d_xy.cpu().numpy().view(np.uint32).reshape(-1, 16), d_inf.cpu().numpy().view(np.uint8)


def device_fft(c, xy, inf, log_n, batch=1, flags=0, stream=None):
    import torch
    d_xy, d_inf = dev(xy), dev(inf)
    torch.cuda.synchronize()  # the arrays were made on torch's stream
    c.g1_fft_device(d_xy.data_ptr(), d_inf.data_ptr(), log_n, batch, flags, stream)
    return host(d_xy, d_inf)


def same(got, want, what=None):
    (xy, inf), (wxy, winf) = got, want
    assert xy.shape == wxy.shape and inf.shape == winf.shape, what
    bad = np.flatnonzero((xy != wxy).any(axis=1) | (inf != winf))
    assert bad.size == 0, (what, "first wrong point", int(bad[0]), "of", xy.shape[0], "wrong", int(bad.size))


@pytest.fixture(scope="module")
def ref():
    """per log_n: seeded logarithms with identities among them, the inputs in both forms and the expected transforms per (direction, output
    form), each computed once on first use; the tests leave them unchanged"""
    cache = {}

    def get(log_n):
        if log_n not in cache:
            a = gc.logs(0x6F1F7 + log_n, 1 << log_n, zero_every=7 if log_n >= 3 else 0)
            cache[log_n] = {"a": a, "in": {0: gc.inputs(a, 0), BS: gc.inputs(a, BS)}, "want": {}}
        return cache[log_n]

    def want(log_n, flags):
        e, key = get(log_n), flags & (INV | OS)
        if key not in e["want"]:
            e["want"][key] = gc.expected(e["a"], log_n, key)
        return e["want"][key]

    get.want = want
    return get


# 1
@pytest.mark.parametrize("flags", gc.FLAG_MATRIX)
@pytest.mark.parametrize("log_n", LOG_NS)
def test_sizes_and_flags(ctx, ref, log_n, flags):
    p = mh.g1_fft_plan(log_n)
    assert p["inv_group"] == 256 and p["stages"] == log_n
    xy, inf = ref(log_n)["in"][flags & BS]
    same(device_fft(ctx, xy, inf, log_n, flags=flags), ref.want(log_n, flags), (log_n, flags))


# 2
@pytest.mark.parametrize("log_n", [3, 9])
def test_batch(ctx, log_n):
    """three arrays in one call: each equals its own single transform, and the bytes after the last array are untouched"""
    n, batch, tail = 1 << log_n, 3, 16
    a = gc.logs(0xBA7C4 + log_n, batch * n, zero_every=5)
    xy, inf = gc.inputs(a)
    padded_xy = np.concatenate([xy, np.full((tail, 16), FILL * 0x01010101, np.uint32)])
    padded_inf = np.concatenate([inf, np.full(tail, FILL, np.uint8)])
    for flags in (0, INV):
        got = device_fft(ctx, padded_xy, padded_inf, log_n, batch, flags)
        assert (got[0][batch * n:] == FILL * 0x01010101).all() and (got[1][batch * n:] == FILL).all(), "the bytes behind the last array"
        for b in range(batch):
            lo, hi = b * n, (b + 1) * n
            single = device_fft(ctx, xy[lo:hi], inf[lo:hi], log_n, 1, flags)
            same((got[0][lo:hi], got[1][lo:hi]), single, (flags, b, "against its own transform"))
        same((got[0][:batch * n], got[1][:batch * n]), gc.expected(a, log_n, flags, batch), (flags, "against the closed form"))


# 3
def test_reference_srs_known_answers(ctx):
    """the halo2 KZG parameter files the reference ships hold g[j] = tau^j * G and g_lagrange[i] = L_i(tau) * G of a tau nobody knows:
    inverse(g) = g_lagrange and forward(g_lagrange) = g, on the Montgomery words as the files store them"""
    sets = gc.srs_sets()
    assert [k for _, k, *_ in sets] == [3, 4]
    for fname, k, omega, g, gl in sets:
        assert omega == mh.fr_root_of_unity(k)
        none = np.zeros(1 << k, np.uint8)
        same(device_fft(ctx, g, none, k, flags=INV), (gl, none), (fname, "inverse(g) = g_lagrange"))
        same(device_fft(ctx, gl, none, k), (g, none), (fname, "forward(g_lagrange) = g"))
        both = device_fft(ctx, np.concatenate([g, gl]), np.zeros(2 << k, np.uint8), k, batch=2, flags=INV)  # (and as a batch)
        assert (both[0][:1 << k] == gl).all()


# 4
@pytest.mark.parametrize("log_n", [4, 9])
def test_identities(ctx, log_n):
    """a constant vector (n * P at index 0, the identity elsewhere: the first stage meets A = T in every butterfly, the way back A = -T), unit
    vectors (outputs w^(mi) * P, every other input flagged), everything flagged, alternating P, -P; the flagged inputs carry garbage words, and
    no flagged place leaks them: the identity comes out as sixteen zero words"""
    n = 1 << log_n
    cases = gc.identity_cases(log_n)
    assert set(cases) == {"constant", "all_flagged", "alternating", "unit_0", "unit_1", "unit_%d" % (n // 2), "unit_%d" % (n - 1)}
    for name, a in cases.items():
        xy, inf = gc.inputs(a)
        assert (xy[inf != 0] == gc.GARBAGE).all()
        for flags in (0, INV):
            got = device_fft(ctx, xy, inf, log_n, flags=flags)
            same(got, gc.expected(a, log_n, flags), (name, flags))
            assert not got[0][got[1] != 0].any() and set(np.unique(got[1])) <= {0, 1}, (name, flags)
            if name == "constant":
                assert list(np.flatnonzero(got[1] == 0)) == [0]
                if flags == INV:  # n^-1 * n * P = P: the input's own words
                    assert (got[0][0] == xy[0]).all()
            if name == "all_flagged":
                assert (got[1] == 1).all() and not got[0].any()
            if name.startswith("unit_"):
                assert not got[1].any()  # w^(mi) * P is never the identity
    # a flag byte other than 1 flags as well, and comes out as 1
    a = gc.logs(0xF1A6, n, zero_every=2)
    xy, inf = gc.inputs(a)
    same(device_fft(ctx, xy, inf * 0xFF, log_n), gc.expected(a, log_n), "flag bytes 0xFF")


# 5
def test_round_trip(ctx, ref):
    """inverse(forward(x)) = x and forward(inverse(x)) = x at 2^12, with identities among the points"""
    import torch
    log_n = 12
    xy, inf = ref(log_n)["in"][0]
    clean = xy.copy()
    clean[inf != 0] = 0  # what the call leaves at an identity
    for first, second in ((0, INV), (INV, 0)):
        d_xy, d_inf = dev(xy), dev(inf)
        torch.cuda.synchronize()
        ctx.g1_fft_device(d_xy.data_ptr(), d_inf.data_ptr(), log_n, 1, first)
        mid = host(d_xy, d_inf)
        same(mid, ref.want(log_n, first), ("half way", first))
        ctx.g1_fft_device(d_xy.data_ptr(), d_inf.data_ptr(), log_n, 1, second)
        same(host(d_xy, d_inf), (clean, inf), ("there and back", first))


# 6
def test_lagrange_basis_from_powers_of_tau(ctx):
    """the use case, on one stream at 2^12: tau^j * G (powers, then the fixed-base call) through the INVERSE group transform is word for word
    L_i(tau) * G (the Lagrange coefficients, then the fixed-base call); the basis then sums to the generator"""
    import torch
    log_n = 12
    n = 1 << log_n
    tau = gc.logs(0x7A0, 1)[0]
    gen = np.concatenate([orc.int_to_words(1), orc.int_to_words(2)])
    d_k, d_l = dev(np.zeros((n, 8), np.uint32)), dev(np.zeros((n, 8), np.uint32))
    d_xy, d_inf = dev(np.full((n, 16), FILL * 0x01010101, np.uint32)), dev(np.full(n, FILL, np.uint8))
    w_xy, w_inf = dev(np.full((n, 16), FILL * 0x01010101, np.uint32)), dev(np.full(n, FILL, np.uint8))
    d_one = dev(np.stack([orc.int_to_words(1)] * n))
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    q = st.cuda_stream
    ctx.fr_powers_device(tau, d_k.data_ptr(), n, stream=q)
    ctx.fixed_base_mul_device(gen, d_k.data_ptr(), n, d_xy.data_ptr(), d_inf.data_ptr(), stream=q)
    ctx.g1_fft_device(d_xy.data_ptr(), d_inf.data_ptr(), log_n, 1, INV, stream=q)
    ctx.fr_lagrange_device(tau, log_n, d_l.data_ptr(), stream=q)
    ctx.fixed_base_mul_device(gen, d_l.data_ptr(), n, w_xy.data_ptr(), w_inf.data_ptr(), stream=q)
    r = ctx.msm_device(d_xy.data_ptr(), d_one.data_ptr(), n, d_inf.data_ptr(), stream=q)
    got = host(d_xy, d_inf)
    same(got, host(w_xy, w_inf), "against the fixed-base call on L_i(tau)")
    assert not got[1].any()
    lag = [pow(tau, n, R) - 1] * 4  # a prefix against Python integers: L_i(tau) = (tau^n - 1) w^i / (n (tau - w^i))
    w = gc.root(log_n)
    lag = [lag[i] * pow(w, i, R) * pow(n * (tau - pow(w, i, R)), -1, R) % R for i in range(4)]
    same((got[0][:4], got[1][:4]), gc.points(lag), "a prefix against the definition")
    assert not r.is_infinity and (r.affine_std == gen).all(), "the Lagrange basis sums to the generator"


# 7
def test_errors_leave_the_context_usable(ctx, ref):
    import torch
    log_n = 3
    n = 1 << log_n
    lib = mh.load_library()
    d_xy, d_inf = dev(np.full((n + 16, 16), FILL * 0x01010101, np.uint32)), dev(np.full(n + 16, FILL, np.uint8))
    torch.cuda.synchronize()
    xy, inf = d_xy.data_ptr(), d_inf.data_ptr()
    bad = [(None, inf, log_n, 1, 0), (xy, None, log_n, 1, 0), (xy + 4, inf, log_n, 1, 0), (xy, inf + 1, log_n, 1, 0), (xy, inf, 29, 1, 0),
           (xy, inf, log_n, 1, 2), (xy, inf, log_n, 1, 4), (xy, inf, log_n, 1, 32), (xy, inf, log_n, 1, 1 << 31), (xy, inf, 28, 1 << 9, 0),
           (xy, inf, 0, (1 << 36) + 1, 0)]
    for args in bad:
        with pytest.raises(mh.MsmError) as e:
            ctx.g1_fft_device(*args)
        assert e.value.code == mh.ERR_BAD_ARG, args
    with pytest.raises(mh.MsmError) as e:
        ctx.g1_fft_device(xy, inf, log_n, 0, 0)
    assert e.value.code == mh.ERR_EMPTY
    assert lib.msm_bn254_g1_fft_device(None, xy, inf, log_n, 1, 0, None) == mh.ERR_BAD_ARG
    h_in = np.ascontiguousarray(ref(log_n)["in"][0][0])
    h_xy, h_inf = np.full((n, 16), FILL * 0x01010101, np.uint32), np.full(n, FILL, np.uint8)
    p32, p8 = lambda a: a.ctypes.data_as(mh._u32p), lambda a: a.ctypes.data_as(mh._u8p)
    for form, k, batch, flags, want in ((2, log_n, 1, 0, mh.ERR_BAD_ARG), (mh.FORM_MONT, log_n, 1, BS, mh.ERR_BAD_ARG), (mh.FORM_MONT, log_n, 1, 2, mh.ERR_BAD_ARG),
                                        (mh.FORM_MONT, 29, 1, 0, mh.ERR_BAD_ARG), (mh.FORM_MONT, log_n, 0, 0, mh.ERR_EMPTY)):
        assert lib.msm_bn254_g1_fft(ctx._h, p32(h_in), form, None, k, batch, flags, p32(h_xy), p8(h_inf)) == want, (form, k, batch, flags)
    for a_in, a_xy, a_inf in ((None, p32(h_xy), p8(h_inf)), (p32(h_in), None, p8(h_inf)), (p32(h_in), p32(h_xy), None)):
        assert lib.msm_bn254_g1_fft(ctx._h, a_in, mh.FORM_MONT, None, log_n, 1, 0, a_xy, a_inf) == mh.ERR_BAD_ARG
    with pytest.raises(mh.MsmError):
        ctx.g1_fft(h_in, log_n + 1)  # not batch * 2^log_n points
    got = host(d_xy, d_inf)
    assert (got[0] == FILL * 0x01010101).all() and (got[1] == FILL).all()  # no failed call wrote anything
    assert (h_xy == FILL * 0x01010101).all() and (h_inf == FILL).all()
    in_xy, in_inf = ref(log_n)["in"][0]
    same(device_fft(ctx, in_xy, in_inf, log_n), ref.want(log_n, 0), "a correct call after the errors")
    same(ctx.g1_fft(in_xy, log_n, mh.FORM_MONT, in_inf, flags=INV), ref.want(log_n, INV), "and a correct host call")


# 8
def test_two_streams(ref):
    """two transforms of different sizes on two streams of one fresh context (each builds its table on its own stream), then each size on the
    OTHER stream (which waits for the build): all four right"""
    import torch
    ka, kb = 9, 7
    (xa, ia), (xb, ib) = ref(ka)["in"][0], ref(kb)["in"][BS]
    with mh.MsmContext() as c:
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        bufs = [(dev(xa), dev(ia)), (dev(xb), dev(ib)), (dev(xa), dev(ia)), (dev(xb), dev(ib))]
        torch.cuda.synchronize()
        c.g1_fft_device(bufs[0][0].data_ptr(), bufs[0][1].data_ptr(), ka, 1, INV, s1.cuda_stream)
        c.g1_fft_device(bufs[1][0].data_ptr(), bufs[1][1].data_ptr(), kb, 1, BS | OS, s2.cuda_stream)
        c.g1_fft_device(bufs[2][0].data_ptr(), bufs[2][1].data_ptr(), ka, 1, 0, s2.cuda_stream)
        c.g1_fft_device(bufs[3][0].data_ptr(), bufs[3][1].data_ptr(), kb, 1, BS | INV, s1.cuda_stream)
        same(host(*bufs[0]), ref.want(ka, INV), "stream 1, 2^9 inverse")
        same(host(*bufs[1]), ref.want(kb, OS), "stream 2, 2^7 forward")
        same(host(*bufs[2]), ref.want(ka, 0), "stream 2, 2^9 forward, table built on stream 1")
        same(host(*bufs[3]), ref.want(kb, INV), "stream 1, 2^7 inverse, table built on stream 2")


# 9
def test_host_form(ctx, ref):
    """pageable arrays, both base forms, inf=None, and in place (out_xy is xy)"""
    log_n = 9
    n = 1 << log_n
    a = gc.logs(0x4057, n)  # no identity among the inputs: inf=None
    for form, in_flag in ((mh.FORM_MONT, 0), (mh.FORM_STD, BS)):
        src, _ = gc.inputs(a, in_flag)
        for flags in (0, INV | OS):
            xy, out_inf = src.copy(), np.full(n, FILL, np.uint8)
            r_xy, r_inf = ctx.g1_fft(xy, log_n, form, None, flags=flags, out_xy=xy, out_inf=out_inf)
            assert r_xy is xy and r_inf is out_inf
            same((xy, out_inf), gc.expected(a, log_n, flags), (form, flags, "in place"))
    xy, inf = ref(log_n)["in"][0]
    keep = xy.copy()
    got = ctx.g1_fft(xy, log_n, mh.FORM_MONT, inf, flags=INV)
    assert (xy == keep).all()  # out of place: the input stays
    same(got, ref.want(log_n, INV), "with a mask, out of place")
    got = ctx.g1_fft(np.concatenate([xy, xy]), log_n, mh.FORM_MONT, np.concatenate([inf, inf]), batch=2)
    same((got[0][n:], got[1][n:]), ref.want(log_n, 0), "a batch of two")
