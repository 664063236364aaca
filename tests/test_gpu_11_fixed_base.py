"""The G1 fixed-base batch multiplication on the GPU (-m gpu): msm_bn254_g1_fixed_base_mul(_device) against the CPU oracle with k reduced modulo r
in Python -- sizes around the inversion group, the edge scalars of every window width, identities at every place of a group, other bases and the
table cache, errors, two streams, and scalars -> bases -> MSM end to end on one stream.  Inputs come from fixed seeds; every comparison is
word-exact."""
import os
import sys

import numpy as np
import pytest

import mopro_msm_hip as mh
from oracle import bn254_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fixed_base_cases as fb  # noqa: E402

pytestmark = pytest.mark.gpu
P, R = fb.P, fb.R
IM, OS = mh.NTT_IN_MONT, mh.FB_OUT_STD
FILL = 0x5A  # every byte of the outputs before a call: a record the kernel skips shows up
G = mh.fixed_base_plan()["inv_group"]  # (host only)
SIZES = sorted({1, 2, 63, 64, 65, G - 1, G, G + 1, 2 * G + 1, 4096})
OTHER = None  # a base that is not the generator, made once


@pytest.fixture(scope="module")
def ctx():
    c = mh.MsmContext()
    yield c
    c.close()


def other_base():
    global OTHER
    if OTHER is None:
        OTHER = fb.point(0xC0FFEE)
    return OTHER


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


def device_mul(c, base, k_words, form=mh.FORM_STD, window_bits=0, flags=0, stream=None):
    import torch
    d_k = dev(k_words)
    d_xy, d_inf = outputs(k_words.shape[0])
    torch.cuda.synchronize()  # the arrays were made on torch's stream
    c.fixed_base_mul_device(base, d_k.data_ptr(), k_words.shape[0], d_xy.data_ptr(), d_inf.data_ptr(), form, window_bits, flags, stream)
    return host(d_xy, d_inf)


def same(got, want, what=None):
    (xy, inf), (wxy, winf) = got, want
    assert xy.shape == wxy.shape and inf.shape == winf.shape, what
    bad = np.flatnonzero((xy != wxy).any(axis=1) | (inf != winf))
    assert bad.size == 0, (what, "first wrong point", int(bad[0]), "of", xy.shape[0], "wrong", int(bad.size))


@pytest.fixture(scope="module")
def ref():
    """4096 seeded 256-bit patterns and what the call must give for them, per flag set, computed once; the tests take prefixes"""
    ks = fb.patterns(0xF1BA5E, 4096)
    inv_mont = pow(fb.MONT_R, -1, R)
    return fb.to_words(ks), {0: fb.expected(ks), OS: fb.expected(ks, out_std=True), IM: fb.expected([k * inv_mont % R for k in ks])}


# 1
@pytest.mark.parametrize("flags", [0, OS, IM])
@pytest.mark.parametrize("n", SIZES)
def test_sizes_around_the_inversion_group(ctx, ref, n, flags):
    words, want = ref
    same(device_mul(ctx, fb.base_words(fb.GEN), words[:n], flags=flags), (want[flags][0][:n], want[flags][1][:n]), (n, flags))


# 2
@pytest.mark.parametrize("c", [4, 8, 13, 16, 0])
def test_edge_scalars_at_every_window_width(ctx, c):
    width = mh.fixed_base_plan(c)["window_bits"]
    ks = fb.edge_scalars(width)
    assert ks[3] == R - 1 and len(ks) > 2 * (256 // width)
    got = device_mul(ctx, fb.base_words(fb.GEN), fb.to_words(ks), window_bits=c, flags=OS)
    same(got, fb.expected(ks, out_std=True), c)
    xy, inf = got
    assert list(inf[:8]) == [1, 0, 0, 0, 1, 0, 1, 1]              # 0, 1, 2, r - 1, r, r + 1, 2r, 5r
    assert orc.words_to_int(xy[1, :8]) == 1 and orc.words_to_int(xy[1, 8:]) == 2
    assert orc.words_to_int(xy[3, :8]) == 1 and orc.words_to_int(xy[3, 8:]) == P - 2  # (r - 1) * G = -G: same x, y = p - y
    assert (xy[5] == xy[1]).all()


# 3
def test_identities_at_every_place_of_a_group(ctx, ref):
    n = 2 * G + 1
    words = ref[0][:n]
    ks = [orc.words_to_int(w) for w in words]
    zeros = [0, R, 2 * R, 5 * R]
    places = {"first of a group": [0, G, 2 * G], "last of a group": [G - 1, 2 * G - 1], "a whole group": list(range(G, 2 * G)),
              "every second lane": list(range(0, n, 2)), "all": list(range(n))}
    for name, at in places.items():
        mixed = list(ks)
        for t, i in enumerate(at):
            mixed[i] = zeros[t % 4]
        xy, inf = device_mul(ctx, fb.base_words(fb.GEN), fb.to_words(mixed))
        hit = np.zeros(n, bool)
        hit[at] = True
        assert (inf[hit] == 1).all() and not xy[hit].any(), name                      # flagged, coordinates all zero
        assert (inf[~hit] == 0).all() and (xy[~hit] == ref[1][0][0][:n][~hit]).all(), name  # every neighbour still exact


# 4
def test_bases_table_cache_and_errors(ctx, ref):
    import torch
    a, b = other_base(), fb.GEN
    ks = fb.patterns(77, 70) + [0, R, R - 1]
    words = fb.to_words(ks)
    want_a, want_b = fb.expected(ks, a), fb.expected(ks, b)
    same(device_mul(ctx, fb.base_words(a), words), want_a, "a non-generator base")
    same(device_mul(ctx, fb.base_words(a, mh.FORM_MONT), words, form=mh.FORM_MONT), want_a, "the base in Montgomery form")
    same(device_mul(ctx, fb.base_words(b), words), want_b, "base B after base A")
    same(device_mul(ctx, fb.base_words(a), words), want_a, "base A again")
    for c in (5, 11, 5):
        same(device_mul(ctx, fb.base_words(a), words, window_bits=c), want_a, ("base A, c changed", c))
    same(device_mul(ctx, fb.base_words(b), words, window_bits=5, flags=OS), fb.expected(ks, b, True), "base B at the width A's table had")
    # errors; the context stays usable
    d_k = dev(words)
    d_xy, d_inf = outputs(len(ks) + 1)
    torch.cuda.synchronize()
    bad = [((fb.base_words((1, 3)),), {}, mh.ERR_INVALID_DATA), ((fb.base_words((0, 0)),), {}, mh.ERR_INVALID_DATA),
           ((np.concatenate([fb.words(P + 1), fb.words(2)]),), {}, mh.ERR_INVALID_DATA),
           ((np.concatenate([fb.words(1), fb.words(P + 2)]),), {}, mh.ERR_INVALID_DATA),
           ((fb.base_words(a, mh.FORM_MONT),), {}, mh.ERR_INVALID_DATA),  # Montgomery words read as standard form: off the curve
           ((fb.base_words(b),), {"form": 2}, mh.ERR_BAD_ARG), ((fb.base_words(b),), {"flags": 1}, mh.ERR_BAD_ARG),
           ((fb.base_words(b),), {"flags": 16}, mh.ERR_BAD_ARG), ((fb.base_words(b),), {"window_bits": 3}, mh.ERR_BAD_ARG),
           ((fb.base_words(b),), {"window_bits": 17}, mh.ERR_BAD_ARG)]
    for (base,), kw, code in bad:
        with pytest.raises(mh.MsmError) as e:
            ctx.fixed_base_mul_device(base, d_k.data_ptr(), len(ks), d_xy.data_ptr(), d_inf.data_ptr(), **kw)
        assert e.value.code == code, (kw, str(e.value))
    with pytest.raises(mh.MsmError) as e:
        ctx.fixed_base_mul_device(fb.base_words(b), d_k.data_ptr(), 0, d_xy.data_ptr(), d_inf.data_ptr())
    assert e.value.code == mh.ERR_EMPTY
    with pytest.raises(mh.MsmError) as e:
        ctx.fixed_base_mul(fb.base_words(b), np.zeros((0, 8), np.uint32))
    assert e.value.code == mh.ERR_EMPTY
    for ptrs in ((d_k.data_ptr(), d_xy.data_ptr() + 4, d_inf.data_ptr()), (d_k.data_ptr() + 8, d_xy.data_ptr(), d_inf.data_ptr()),
                 (d_k.data_ptr(), d_xy.data_ptr(), d_inf.data_ptr() + 1), (None, d_xy.data_ptr(), d_inf.data_ptr()),
                 (d_k.data_ptr(), None, d_inf.data_ptr()), (d_k.data_ptr(), d_xy.data_ptr(), None)):
        with pytest.raises(mh.MsmError) as e:
            ctx.fixed_base_mul_device(fb.base_words(b), ptrs[0], len(ks), ptrs[1], ptrs[2])
        assert e.value.code == mh.ERR_BAD_ARG, ptrs
    got = host(d_xy, d_inf)
    assert (got[0] == FILL * 0x01010101).all() and (got[1] == FILL).all()  # no failed call wrote anything
    same(device_mul(ctx, fb.base_words(a), words), want_a, "a correct call after the errors")
    same(device_mul(ctx, fb.base_words(fb.GEN), ref[0][:100]), (ref[1][0][0][:100], ref[1][0][1][:100]), "and the default table again")


# 5
def test_two_streams(ctx, ref):
    import torch
    n = 2 * G + 1
    words = ref[0][:n]
    a = other_base()
    ks = [orc.words_to_int(w) for w in words[:40]]
    d_k = dev(words)
    xy1, inf1 = outputs(n)
    xy2, inf2 = outputs(40)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    ctx.fixed_base_mul_device(fb.base_words(fb.GEN), d_k.data_ptr(), n, xy1.data_ptr(), inf1.data_ptr(), stream=s1.cuda_stream)
    ctx.fixed_base_mul_device(fb.base_words(a), d_k.data_ptr(), 40, xy2.data_ptr(), inf2.data_ptr(), stream=s2.cuda_stream)  # rebuilds the table
    ctx.fixed_base_mul_device(fb.base_words(a), d_k.data_ptr(), 40, xy2.data_ptr(), inf2.data_ptr(), flags=OS, stream=s1.cuda_stream)
    same(host(xy1, inf1), (ref[1][0][0][:n], ref[1][0][1][:n]), "stream 1")
    same(host(xy2, inf2), fb.expected(ks, a, True), "stream 2, then stream 1 again")


# 6
def test_host_pointer_form_equals_device_form(ctx, ref):
    n = 2 * G + 1
    for flags in (0, OS, IM):
        xy, inf = ctx.fixed_base_mul(fb.base_words(fb.GEN), ref[0][:n], flags=flags)
        same((xy, inf), device_mul(ctx, fb.base_words(fb.GEN), ref[0][:n], flags=flags), flags)
        same((xy, inf), (ref[1][flags][0][:n], ref[1][flags][1][:n]), flags)


# 7
def test_scalars_to_bases_to_msm_in_hbm(ctx):
    """k_i -> k_i * G as Montgomery words in HBM -> msm_bn254_g1_device with scalars s_i, one stream, nothing crossing PCIe in between"""
    import torch
    n = 4096
    k, s = orc.gen_scalars(0xB2540011, n, nonzero=True), orc.gen_scalars(0xB2540012, n)
    k[5] = 0  # one identity among the bases: it travels as d_inf_mask
    d_k, d_s = dev(k), dev(s)
    d_xy, d_inf = outputs(n)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    ctx.fixed_base_mul_device(fb.base_words(fb.GEN), d_k.data_ptr(), n, d_xy.data_ptr(), d_inf.data_ptr(), stream=st.cuda_stream)
    r = ctx.msm_device(d_xy.data_ptr(), d_s.data_ptr(), n, d_inf.data_ptr(), stream=st.cuda_stream)
    want, winf = orc.closed_form_expected(k, s)
    assert not winf and not r.is_infinity and (r.affine_std == want).all()
    assert host(d_xy, d_inf)[1].sum() == 1


# 8
def test_against_the_hooks_generator():
    """the test hook that made such points before (254 one-bit windows, one inversion per point) gives the same words"""
    from mopro_msm_hip import testhooks
    if not os.path.exists(testhooks.HOOKS_LIB_PATH):
        pytest.skip("the hooks library is not built")
    n, seed = 1000, 0xB2540021
    with testhooks.HooksContext() as h:
        d_b = dev(np.zeros((n, 16), np.uint32))
        h.generate_device(seed, 0, n, d_b.data_ptr(), None)
        hook = host(d_b, dev(np.zeros(n, np.uint8)))[0]
        same(device_mul(h, fb.base_words(fb.GEN), orc.gen_scalars(seed, n, nonzero=True)), (hook, np.zeros(n, np.uint8)), "hook")


# 9
def test_the_staging_boundary_of_the_host_form(ctx, ref):
    """2^20 + 513 scalars: the host-pointer form stages 2^20 at a time, so its loop runs twice"""
    n = (1 << 20) + 513
    reps = -(-n // 513)
    words = np.tile(ref[0][:513], (reps, 1))[:n]
    want = (np.tile(ref[1][0][0][:513], (reps, 1))[:n], np.tile(ref[1][0][1][:513], reps)[:n])
    same(ctx.fixed_base_mul(fb.base_words(fb.GEN), words), want, "host form")
