"""The G2 group transform on the GPU (-m gpu): msm_bn254_g2_fft(_device) against the closed form of tools/g2_fft_cases.py -- the points of the Fr
transform of the inputs' logarithms, from the independent Python G2 law -- at sizes below a wavefront, below, at and above a workgroup of
butterflies, under every flag, in batches, against the G2 MSM as the definition, on the structured vectors whose butterflies double, cancel and
meet the identity, there and back, as the step from the tauG2 section to the Lagrange basis on one stream, with input that is not in G2 among
live arrays, after every error, on two streams, through the host form, and sharing its twiddle table with the G1 transform.  Inputs come from
fixed seeds; every comparison is word-exact."""
import os
import sys

import numpy as np
import pytest

import mopro_msm_hip as mh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import g2_fft_cases as gc  # noqa: E402

pytestmark = pytest.mark.gpu
P, R = gc.P, gc.R
g2, fb2, g1c = gc.g2, gc.fb2, gc.g1c
INV, OS, BS = gc.INVERSE, gc.OUT_STD, gc.IN_STD
FILL = 0x5A  # every byte of an output before a call: a record the kernel skips, or one it must not touch, shows up
G = 256      # butterflies of a workgroup; test_sizes_and_flags checks it against the plan
LOG_NS = [0, 1, 2, 3, 7, 8, 9, 10]  # butterflies: none, 1 .. 4 (below a wavefront), 64, 128 (below a workgroup), 256 (one), 512 (two)


@pytest.fixture(scope="module")
def ctx():
    c = mh.MsmContext()
    yield c
    c.close()


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32 if a.dtype == np.uint32 else np.uint8).copy()).to("cuda:0")


def host(d_xy, d_inf, width=32):
    import torch
    torch.cuda.synchronize()
    return d_xy.cpu().numpy().view(np.uint32).reshape(-1, width), d_inf.cpu().numpy().view(np.uint8)


def device_fft(c, xy, inf, log_n, batch=1, flags=0, stream=None):
    import torch
    d_xy, d_inf = dev(xy), dev(inf)
    torch.cuda.synchronize()  # the arrays were made on torch's stream
    c.g2_fft_device(d_xy.data_ptr(), d_inf.data_ptr(), log_n, batch, flags, stream)
    return host(d_xy, d_inf)


def same(got, want, what=None):
    (xy, inf), (wxy, winf) = got, want
    assert xy.shape == wxy.shape and inf.shape == winf.shape, what
    bad = np.flatnonzero((xy != wxy).any(axis=1) | (inf != winf))
    assert bad.size == 0, (what, "first wrong point", int(bad[0]), "of", xy.shape[0], "wrong", int(bad.size))


@pytest.fixture(scope="module")
def ref():
    """per log_n: seeded logarithms with an identity at every 7th place, the inputs in both forms and the expected transforms per (direction,
    output form), each computed once on first use; the tests leave them unchanged"""
    cache = {}

    def get(log_n):
        if log_n not in cache:
            a = gc.logs(0x62F1F7 + log_n, 1 << log_n, zero_every=7 if log_n >= 3 else 0)
            cache[log_n] = {"a": a, "in": {}, "want": {}}
        return cache[log_n]

    def inputs(log_n, in_flag=0):
        e = get(log_n)
        if in_flag not in e["in"]:
            e["in"][in_flag] = gc.inputs(e["a"], in_flag)
        return e["in"][in_flag]

    def want(log_n, flags):
        e, key = get(log_n), flags & (INV | OS)
        if key not in e["want"]:
            e["want"][key] = gc.expected(e["a"], log_n, key)
        return e["want"][key]

    get.inputs, get.want = inputs, want
    return get


# 1
@pytest.mark.parametrize("flags", gc.FLAG_MATRIX)
@pytest.mark.parametrize("log_n", LOG_NS)
def test_sizes_and_flags(ctx, ref, log_n, flags):
    """from stage 9 on a butterfly's two records lie a workgroup of butterflies apart"""
    p = mh.g2_fft_plan(log_n)
    assert p["inv_group"] == G and p["stages"] == log_n
    xy, inf = ref.inputs(log_n, flags & BS)
    if log_n >= 3:
        assert inf[1::7].all() and inf.sum() == len(range(1, 1 << log_n, 7)) and (xy[inf != 0] == gc.GARBAGE).all()
    same(device_fft(ctx, xy, inf, log_n, flags=flags), ref.want(log_n, flags), (log_n, flags))


# 2
@pytest.mark.parametrize("log_n", [3, 9])
def test_batch(ctx, log_n):
    """three arrays in one call: each equals its own single transform and the closed form, and the bytes after the last array are untouched"""
    n, batch, tail = 1 << log_n, 3, 16
    a = gc.logs(0xBA7C42 + log_n, batch * n, zero_every=5)
    xy, inf = gc.inputs(a)
    padded_xy = np.concatenate([xy, np.full((tail, 32), FILL * 0x01010101, np.uint32)])
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
def test_the_definition_through_the_g2_msm(ctx, ref):
    """log_n = 4: output i is sum_j w^(+-ij) * Q_j (times n^-1 on the way back) -- sixteen calls of msm_bn254_g2_device on the same 16 points"""
    import torch
    log_n = 4
    n = 1 << log_n
    xy, inf = ref.inputs(log_n)
    assert inf.any()
    w = gc.root(log_n)
    d_xy, d_inf = dev(xy), dev(inf)
    for flags in (0, INV):
        ww, scale = (pow(w, -1, R), pow(n, -1, R)) if flags else (w, 1)
        got = device_fft(ctx, xy, inf, log_n, flags=flags | OS)
        same(got, ref.want(log_n, flags | OS), ("against the cases", flags))
        for i in range(n):
            d_s = dev(fb2.to_words([scale * pow(ww, i * j, R) % R for j in range(n)]))
            torch.cuda.synchronize()
            r = ctx.msm_g2_device(d_xy.data_ptr(), d_s.data_ptr(), n, d_inf.data_ptr())
            if r.is_infinity:
                assert got[1][i] == 1 and not got[0][i].any(), (flags, i)
            else:
                x, y = r.affine_ints()
                assert got[1][i] == 0 and gc.point_ints(got[0][i]) == x + y, (flags, i)


# 4
@pytest.mark.parametrize("log_n", [4, 9])
def test_identities(ctx, log_n):
    """a constant vector (n * Q at index 0, the identity elsewhere: the first stage meets A = T in every butterfly, the way back A = -T), unit
    vectors (outputs w^(mi) * Q, every other input flagged), everything flagged, alternating Q, -Q; the flagged inputs carry garbage words, and
    no flagged place leaks them: the identity comes out as 32 zero words"""
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
                if flags == INV:  # n^-1 * n * Q = Q: the input's own words
                    assert (got[0][0] == xy[0]).all()
            if name == "all_flagged":
                assert (got[1] == 1).all() and not got[0].any()
            if name.startswith("unit_"):
                assert not got[1].any()  # w^(mi) * Q is never the identity
    # a flag byte other than 1 flags as well, and comes out as 1
    a = gc.logs(0xF1A6, n, zero_every=2)
    xy, inf = gc.inputs(a)
    same(device_fft(ctx, xy, inf * 0xFF, log_n), gc.expected(a, log_n), "flag bytes 0xFF")


# 5
def test_round_trip(ctx, ref):
    """inverse(forward(x)) = x and forward(inverse(x)) = x at 2^12, with identities among the points"""
    import torch
    log_n = 12
    xy, inf = ref.inputs(log_n)
    assert inf.any()
    clean = xy.copy()
    clean[inf != 0] = 0  # what the call leaves at an identity
    for first, second in ((0, INV), (INV, 0)):
        d_xy, d_inf = dev(xy), dev(inf)
        torch.cuda.synchronize()
        ctx.g2_fft_device(d_xy.data_ptr(), d_inf.data_ptr(), log_n, 1, first)
        mid = host(d_xy, d_inf)
        same(mid, ref.want(log_n, first), ("half way", first))
        ctx.g2_fft_device(d_xy.data_ptr(), d_inf.data_ptr(), log_n, 1, second)
        same(host(d_xy, d_inf), (clean, inf), ("there and back", first))


# 6
def test_lagrange_basis_from_the_tau_g2_section(ctx):
    """the use case, on one non-default stream at 2^12: tau^j * H (powers, then the G2 fixed-base call) through the INVERSE group transform is
    word for word L_i(tau) * H (the Lagrange coefficients, then the fixed-base call); the result is in G2 and sums to the generator"""
    import torch
    log_n = 12
    n = 1 << log_n
    tau = gc.logs(0x7A02, 1)[0]
    gen = fb2.base_words(gc.GEN)
    d_k, d_l = dev(np.zeros((n, 8), np.uint32)), dev(np.zeros((n, 8), np.uint32))
    d_xy, d_inf = dev(np.full((n, 32), FILL * 0x01010101, np.uint32)), dev(np.full(n, FILL, np.uint8))
    w_xy, w_inf = dev(np.full((n, 32), FILL * 0x01010101, np.uint32)), dev(np.full(n, FILL, np.uint8))
    d_one = dev(fb2.to_words([1] * n))
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    q = st.cuda_stream
    ctx.fr_powers_device(tau, d_k.data_ptr(), n, stream=q)
    ctx.fixed_base_g2_mul_device(gen, d_k.data_ptr(), n, d_xy.data_ptr(), d_inf.data_ptr(), stream=q)
    ctx.g2_fft_device(d_xy.data_ptr(), d_inf.data_ptr(), log_n, 1, INV, stream=q)
    ctx.fr_lagrange_device(tau, log_n, d_l.data_ptr(), stream=q)
    ctx.fixed_base_g2_mul_device(gen, d_l.data_ptr(), n, w_xy.data_ptr(), w_inf.data_ptr(), stream=q)
    assert ctx.validate_g2_device(d_xy.data_ptr(), n, d_inf_ptr=d_inf.data_ptr(), checks=mh.G2_CHECK_SUBGROUP, stream=q) is None
    r = ctx.msm_g2_device(d_xy.data_ptr(), d_one.data_ptr(), n, d_inf.data_ptr(), stream=q)
    got = host(d_xy, d_inf)
    same(got, host(w_xy, w_inf), "against the fixed-base call on L_i(tau)")
    assert not got[1].any()
    w = gc.root(log_n)
    lag = [(pow(tau, n, R) - 1) * pow(w, i, R) * pow(n * (tau - pow(w, i, R)), -1, R) % R for i in range(4)]  # L_i(tau) in Python integers
    same((got[0][:4], got[1][:4]), fb2.expected(lag), "a prefix against the definition")
    assert not r.is_infinity and r.affine_ints() == gc.GEN, "the Lagrange basis sums to the generator"


# 7
@pytest.mark.parametrize("log_n", [1, 2])
def test_input_that_is_not_in_g2_among_live_arrays(ctx, log_n):
    """A batch of G + 1 arrays of 2 resp. 4 points: its butterflies fill two workgroups and start a third, so butterflies of different arrays
    share a workgroup's inversions (at log_n = 1 the plain stage's, at log_n = 2 the ladder stage's as well).  Some arrays hold one record that
    is not in G2 -- a twist point outside the subgroup, arbitrary words above p, a record with x = 0.  WHICH OUTPUTS DEPEND ON IT: after log_n
    stages every output of a transform depends on every input, so all n places of the bad record's own array are meaningless and nothing is
    asserted about their words (their flag bytes are 0 or 1); every place of every other array shares no butterfly with it and must be exact.
    Nothing faults: the call returns and the context goes on working."""
    n, batch = 1 << log_n, G + 1
    a = gc.logs(0x0FF62 + log_n, batch * n, zero_every=9)
    xy, inf = gc.inputs(a)
    want = gc.expected(a, log_n, 0, batch)
    off = fb2.off_subgroup_point()
    assert g2.on_curve(off) and g2.mul_raw(off, R) is not None
    junk = np.tile(np.asarray(fb2.words(fb2.patterns(0xBAD, 1)[0]), np.uint32), 4) | np.uint32(0x80000000)  # every component above p
    x_zero = xy[0].copy()
    x_zero[:16] = 0
    records = [np.array(g2.point_words(off, True), np.uint32), junk, x_zero]
    bad_arrays = sorted({1, 2, 63, G // n - 1, G // n, G // 2, G - 1, G})  # first, inner and last lanes of the workgroups, and the tail
    hit = np.zeros(batch * n, bool)
    for t, b in enumerate(bad_arrays):
        at = b * n + t % n
        xy[at], inf[at] = records[t % 3], 0
        hit[b * n:(b + 1) * n] = True
    for flags in (0, INV):
        got = device_fft(ctx, xy, inf, log_n, batch, flags)
        w = want if flags == 0 else gc.expected(a, log_n, INV, batch)
        assert set(np.unique(got[1][hit])) <= {0, 1}
        assert (got[1][~hit] == w[1][~hit]).all() and (got[0][~hit] == w[0][~hit]).all(), flags
    clean = gc.inputs(a)
    same(device_fft(ctx, clean[0], clean[1], log_n, batch), want, "a clean call afterwards")


# 8
def test_errors_write_nothing_and_leave_the_context_usable(ctx, ref):
    import torch
    log_n = 3
    n = 1 << log_n
    lib = mh.load_library()
    d_xy, d_inf = dev(np.full((n + 16, 32), FILL * 0x01010101, np.uint32)), dev(np.full(n + 16, FILL, np.uint8))
    torch.cuda.synchronize()
    xy, inf = d_xy.data_ptr(), d_inf.data_ptr()
    in_xy, in_inf = ref.inputs(log_n)

    def good(what):
        same(device_fft(ctx, in_xy, in_inf, log_n), ref.want(log_n, 0), what)

    bad = [(None, inf, log_n, 1, 0), (xy, None, log_n, 1, 0), (xy + 4, inf, log_n, 1, 0), (xy, inf + 1, log_n, 1, 0), (xy, inf, 29, 1, 0),
           (xy, inf, log_n, 1, 2), (xy, inf, log_n, 1, 4), (xy, inf, log_n, 1, 32), (xy, inf, log_n, 1, 1 << 31), (xy, inf, 28, 1 << 9, 0),
           (xy, inf, 0, (1 << 36) + 1, 0)]
    for args in bad:
        with pytest.raises(mh.MsmError) as e:
            ctx.g2_fft_device(*args)
        assert e.value.code == mh.ERR_BAD_ARG, args
        good(("a correct call after", args))
    with pytest.raises(mh.MsmError) as e:
        ctx.g2_fft_device(xy, inf, log_n, 0, 0)
    assert e.value.code == mh.ERR_EMPTY
    good("a correct call after batch = 0")
    assert lib.msm_bn254_g2_fft_device(None, xy, inf, log_n, 1, 0, None) == mh.ERR_BAD_ARG
    h_in = np.ascontiguousarray(in_xy)
    h_xy, h_inf = np.full((n, 32), FILL * 0x01010101, np.uint32), np.full(n, FILL, np.uint8)
    p32, p8 = lambda a: a.ctypes.data_as(mh._u32p), lambda a: a.ctypes.data_as(mh._u8p)
    for form, k, batch, flags, want in ((2, log_n, 1, 0, mh.ERR_BAD_ARG), (mh.FORM_MONT, log_n, 1, BS, mh.ERR_BAD_ARG), (mh.FORM_MONT, log_n, 1, 2, mh.ERR_BAD_ARG),
                                        (mh.FORM_MONT, 29, 1, 0, mh.ERR_BAD_ARG), (mh.FORM_MONT, log_n, 0, 0, mh.ERR_EMPTY)):
        assert lib.msm_bn254_g2_fft(ctx._h, p32(h_in), form, None, k, batch, flags, p32(h_xy), p8(h_inf)) == want, (form, k, batch, flags)
        same(ctx.g2_fft(in_xy, log_n, mh.FORM_MONT, in_inf, flags=INV), ref.want(log_n, INV), ("a correct host call after", form, k, batch, flags))
    for a_in, a_xy, a_inf in ((None, p32(h_xy), p8(h_inf)), (p32(h_in), None, p8(h_inf)), (p32(h_in), p32(h_xy), None)):
        assert lib.msm_bn254_g2_fft(ctx._h, a_in, mh.FORM_MONT, None, log_n, 1, 0, a_xy, a_inf) == mh.ERR_BAD_ARG
    with pytest.raises(mh.MsmError):
        ctx.g2_fft(h_in, log_n + 1)  # not batch * 2^log_n points
    got = host(d_xy, d_inf)
    assert (got[0] == FILL * 0x01010101).all() and (got[1] == FILL).all()  # no failed call wrote anything
    assert (h_xy == FILL * 0x01010101).all() and (h_inf == FILL).all()
    good("a correct call after the errors")


# 9
def test_two_streams(ref):
    """two transforms of different sizes on two streams of one fresh context (each builds its table on its own stream), then each size on the
    OTHER stream (which waits for the build): all four right"""
    import torch
    ka, kb = 9, 7
    (xa, ia), (xb, ib) = ref.inputs(ka), ref.inputs(kb, BS)
    with mh.MsmContext() as c:
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        bufs = [(dev(xa), dev(ia)), (dev(xb), dev(ib)), (dev(xa), dev(ia)), (dev(xb), dev(ib))]
        torch.cuda.synchronize()
        c.g2_fft_device(bufs[0][0].data_ptr(), bufs[0][1].data_ptr(), ka, 1, INV, s1.cuda_stream)
        c.g2_fft_device(bufs[1][0].data_ptr(), bufs[1][1].data_ptr(), kb, 1, BS | OS, s2.cuda_stream)
        c.g2_fft_device(bufs[2][0].data_ptr(), bufs[2][1].data_ptr(), ka, 1, 0, s2.cuda_stream)
        c.g2_fft_device(bufs[3][0].data_ptr(), bufs[3][1].data_ptr(), kb, 1, BS | INV, s1.cuda_stream)
        same(host(*bufs[0]), ref.want(ka, INV), "stream 1, 2^9 inverse")
        same(host(*bufs[1]), ref.want(kb, OS), "stream 2, 2^7 forward")
        same(host(*bufs[2]), ref.want(ka, 0), "stream 2, 2^9 forward, table built on stream 1")
        same(host(*bufs[3]), ref.want(kb, INV), "stream 1, 2^7 inverse, table built on stream 2")


# 10
def test_host_form_equals_device_form(ref):
    """pageable arrays, both base forms, inf=None, in place (out_xy is xy), and on a fresh context a small size, a larger one (the staging
    arrays grow) and the small one again"""
    log_n = 7
    n = 1 << log_n
    a = gc.logs(0x40572, n)  # no identity among the inputs: inf=None
    with mh.MsmContext() as c:
        xy3, inf3 = ref.inputs(3)
        same(c.g2_fft(xy3, 3, mh.FORM_MONT, inf3), ref.want(3, 0), "2^3 before the staging arrays grow")
        for form, in_flag in ((mh.FORM_MONT, 0), (mh.FORM_STD, BS)):
            src, none = gc.inputs(a, in_flag)
            assert not none.any()
            for flags in (0, INV | OS):
                xy, out_inf = src.copy(), np.full(n, FILL, np.uint8)
                r_xy, r_inf = c.g2_fft(xy, log_n, form, None, flags=flags, out_xy=xy, out_inf=out_inf)
                assert r_xy is xy and r_inf is out_inf
                same((xy, out_inf), device_fft(c, src, none, log_n, flags=flags | in_flag), (form, flags, "against the device form"))
                same((xy, out_inf), gc.expected(a, log_n, flags), (form, flags, "in place, against the cases"))
        same(c.g2_fft(xy3, 3, mh.FORM_MONT, inf3, flags=INV), ref.want(3, INV), "2^3 after they grew")
        xy, inf = ref.inputs(9)
        keep = xy.copy()
        got = c.g2_fft(xy, 9, mh.FORM_MONT, inf, flags=INV)
        assert (xy == keep).all()  # out of place: the input stays
        same(got, ref.want(9, INV), "2^9 with a mask, out of place: the arrays grow once more")
        got = c.g2_fft(np.concatenate([xy3, xy3]), 3, mh.FORM_MONT, np.concatenate([inf3, inf3]), batch=2)
        same((got[0][8:], got[1][8:]), ref.want(3, 0), "a batch of two")


# 11
def test_one_table_for_both_groups(ref):
    """a G1 transform and then a G2 transform of the same log_n on one fresh context (the G2 call finds the table the G1 call built), and the
    other order on a second context: all four right; the plans name the same table"""
    log_n = 7
    n = 1 << log_n
    assert mh.g1_fft_plan(log_n)["table_bytes"] == mh.g2_fft_plan(log_n)["table_bytes"] == 32 * (n // 2)
    a1 = g1c.logs(0x6162 + log_n, n, zero_every=7)
    in1, want1 = g1c.inputs(a1), g1c.expected(a1, log_n, INV)
    xy2, inf2 = ref.inputs(log_n)

    def g1(c):
        import torch
        d_xy, d_inf = dev(in1[0]), dev(in1[1])
        torch.cuda.synchronize()
        c.g1_fft_device(d_xy.data_ptr(), d_inf.data_ptr(), log_n, 1, INV)
        return host(d_xy, d_inf, 16)

    with mh.MsmContext() as c:
        same(g1(c), want1, "G1 first")
        same(device_fft(c, xy2, inf2, log_n), ref.want(log_n, 0), "G2 on the table the G1 call built")
    with mh.MsmContext() as c:
        same(device_fft(c, xy2, inf2, log_n, flags=INV), ref.want(log_n, INV), "G2 first")
        same(g1(c), want1, "G1 on the table the G2 call built")
