"""The G2 fixed-base batch multiplication on the GPU (-m gpu): msm_bn254_g2_fixed_base_mul(_device) against the Python model of
tools/fixed_base_g2_cases.py (built on tools/bn254_g2_py.py, never on the library) -- sizes around a chain and a wave of chains, the edge
scalars of every window width, identities at every place of a chain, the chunk boundary, other bases and the table cache, errors, two streams,
the G1 table beside the G2 one, and scalars -> G2 bases -> G2 MSM end to end on one stream.  Inputs come from fixed seeds; every comparison is
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
import fixed_base_g2_cases as fb2  # noqa: E402

pytestmark = pytest.mark.gpu
g2 = fb2.g2
P, R = fb2.P, fb2.R
IM, OS = mh.NTT_IN_MONT, mh.FB_OUT_STD
FILL = 0x5A  # every byte of the outputs before a call: a record the kernels skip shows up
PLAN = mh.fixed_base_g2_plan()  # (host only)
G = PLAN["inv_group"]
SIZES = sorted({min(n, 4096) for n in (1, 2, 63, 64, 65, G - 1, G, G + 1, 64 * G - 1, 64 * G + 1, 4096) if n >= 1})
GEN = g2.G2_GEN
OTHER = None  # a base that is not the generator, made once


@pytest.fixture(scope="module")
def ctx():
    c = mh.MsmContext()
    yield c
    c.close()


def other_base():
    global OTHER
    if OTHER is None:
        OTHER = g2.mul(GEN, 0xC0FFEE)
    return OTHER


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32 if a.dtype == np.uint32 else np.uint8).copy()).to("cuda:0")


def outputs(n, words=32):
    return dev(np.full((n, words), FILL * 0x01010101, np.uint32)), dev(np.full(n, FILL, np.uint8))


def host(d_xy, d_inf, words=32):
    import torch
    torch.cuda.synchronize()
    return d_xy.cpu().numpy().view(np.uint32).reshape(-1, words), d_inf.cpu().numpy().view(np.uint8)


def device_mul(c, base, k_words, form=mh.FORM_STD, window_bits=0, flags=0, stream=None):
    import torch
    d_k = dev(k_words)
    d_xy, d_inf = outputs(k_words.shape[0])
    torch.cuda.synchronize()  # the arrays were made on torch's stream
    c.fixed_base_g2_mul_device(base, d_k.data_ptr(), k_words.shape[0], d_xy.data_ptr(), d_inf.data_ptr(), form, window_bits, flags, stream)
    return host(d_xy, d_inf)


def same(got, want, what=None):
    (xy, inf), (wxy, winf) = got, want
    assert xy.shape == wxy.shape and inf.shape == winf.shape, what
    bad = np.flatnonzero((xy != wxy).any(axis=1) | (inf != winf))
    assert bad.size == 0, (what, "first wrong point", int(bad[0]), "of", xy.shape[0], "wrong", int(bad.size))


@pytest.fixture(scope="module")
def ref():
    """4096 seeded 256-bit patterns and what the call must give for them, per flag set, computed once; the tests take prefixes"""
    ks = fb2.patterns(0xF1BA5E2, 4096)
    inv_mont = pow(fb2.MONT_R, -1, R)
    return fb2.to_words(ks), {0: fb2.expected(ks), OS: fb2.expected(ks, out_std=True), IM: fb2.expected([k * inv_mont % R for k in ks])}


# 1
@pytest.mark.parametrize("flags", [0, OS, IM])
@pytest.mark.parametrize("n", SIZES)
def test_sizes_around_a_chain_and_a_wave_of_chains(ctx, ref, n, flags):
    words, want = ref
    same(device_mul(ctx, fb2.base_words(GEN), words[:n], flags=flags), (want[flags][0][:n], want[flags][1][:n]), (n, flags))


# 2
@pytest.mark.parametrize("c", [4, 8, 13, 16, 0])
def test_edge_scalars_at_every_window_width(ctx, c):
    width = mh.fixed_base_g2_plan(c)["window_bits"]
    ks = fb2.edge_scalars(width)
    assert ks[:8] == [0, 1, 2, R - 1, R, R + 1, 2 * R, 5 * R] and len(ks) > 2 * (256 // width)
    got = device_mul(ctx, fb2.base_words(GEN), fb2.to_words(ks), window_bits=c, flags=OS)
    same(got, fb2.expected(ks, out_std=True), c)
    xy, inf = got
    assert list(inf[:8]) == [1, 0, 0, 0, 1, 0, 1, 1]              # 0, 1, 2, r - 1, r, r + 1, 2r, 5r
    gen = np.array(g2.point_words(GEN), np.uint32)
    assert (xy[1] == gen).all()
    neg = np.array(g2.point_words(g2.neg(GEN)), np.uint32)          # (r - 1) * H = -H: same x, both components of y negated
    assert (xy[3][:16] == gen[:16]).all() and (xy[3] == neg).all()
    assert (xy[5] == xy[1]).all()


# 3
def test_identities_at_every_place_of_a_chain_and_a_wave(ctx, ref):
    n = 2 * 64 * G + 1
    words = ref[0][:n]
    ks = [orc.words_to_int(w) for w in words]
    zeros = [0, R, 2 * R, 5 * R]
    chain = [64 * G + 3 + 64 * s for s in range(G)]  # the chain of lane 3 of the second wave
    places = {"first of a chain": [0, chain[0], 2 * 64 * G], "last of a chain": [64 * (G - 1), chain[-1]], "a whole chain": chain,
              "a whole wave step": list(range(64, 128)), "every second point": list(range(0, n, 2)), "all": list(range(n))}
    for name, at in places.items():
        mixed = list(ks)
        for t, i in enumerate(at):
            mixed[i] = zeros[t % 4]
        xy, inf = device_mul(ctx, fb2.base_words(GEN), fb2.to_words(mixed))
        hit = np.zeros(n, bool)
        hit[at] = True
        assert (inf[hit] == 1).all() and not xy[hit].any(), name                      # flagged, coordinates all zero
        assert (inf[~hit] == 0).all() and (xy[~hit] == ref[1][0][0][:n][~hit]).all(), name  # every neighbour still exact


# 4
def test_the_chunk_boundary_on_both_forms(ctx, ref):
    n = PLAN["chunk_points"] + 513
    reps = -(-n // 513)
    words = np.tile(ref[0][:513], (reps, 1))[:n]
    want = (np.tile(ref[1][0][0][:513], (reps, 1))[:n], np.tile(ref[1][0][1][:513], reps)[:n])
    same(device_mul(ctx, fb2.base_words(GEN), words), want, "device form")
    same(ctx.fixed_base_g2_mul(fb2.base_words(GEN), words), want, "host form")


# 5
def test_bases_table_cache_and_errors(ctx, ref):
    import torch
    a, b = other_base(), GEN
    ks = fb2.patterns(77, 70) + [0, R, R - 1]
    words = fb2.to_words(ks)
    want_a, want_b = fb2.expected(ks, a), fb2.expected(ks, b)
    same(device_mul(ctx, fb2.base_words(a), words), want_a, "a non-generator base")
    same(device_mul(ctx, fb2.base_words(a, mh.FORM_MONT), words, form=mh.FORM_MONT), want_a, "the base in Montgomery form")
    same(device_mul(ctx, fb2.base_words(b), words), want_b, "base B after base A")
    same(device_mul(ctx, fb2.base_words(a), words), want_a, "base A again")
    for c in (5, 11, 5):
        same(device_mul(ctx, fb2.base_words(a), words, window_bits=c), want_a, ("base A, c changed", c))
    same(device_mul(ctx, fb2.base_words(b), words, window_bits=5, flags=OS), fb2.expected(ks, b, True), "base B at the width A's table had")
    same(device_mul(ctx, fb2.base_words(a), words, window_bits=5), want_a, "base A: the table the errors must leave in place")
    # errors; the context stays usable
    d_k = dev(words)
    d_xy, d_inf = outputs(len(ks) + 1)
    torch.cuda.synchronize()
    off = fb2.off_subgroup_point()
    assert g2.on_curve(off) and not g2.in_subgroup(off)
    (x0, x1), (y0, y1) = b
    w = fb2.words
    bad = [((fb2.base_words(off),), {}, mh.ERR_INVALID_DATA, "subgroup"),                             # on the twist, outside G2
           ((fb2.base_words(off, mh.FORM_MONT),), {"form": mh.FORM_MONT}, mh.ERR_INVALID_DATA, "subgroup"),
           ((fb2.base_words(((x0, x1), (y0, (y1 + 1) % P))),), {}, mh.ERR_INVALID_DATA, "curve"),   # off the curve
           ((np.zeros(32, np.uint32),), {}, mh.ERR_INVALID_DATA, "curve"),
           ((np.concatenate([w(x0 + P), w(x1), w(y0), w(y1)]),), {}, mh.ERR_INVALID_DATA, "curve"),  # a component >= p
           ((np.concatenate([w(x0), w(x1), w(y0), w(P)]),), {}, mh.ERR_INVALID_DATA, "curve"),
           ((fb2.base_words(a, mh.FORM_MONT),), {}, mh.ERR_INVALID_DATA, "curve"),  # Montgomery words read as standard form: off the curve
           ((fb2.base_words(b),), {"form": 2}, mh.ERR_BAD_ARG, ""), ((fb2.base_words(b),), {"flags": 1}, mh.ERR_BAD_ARG, ""),
           ((fb2.base_words(b),), {"flags": 16}, mh.ERR_BAD_ARG, ""), ((fb2.base_words(b),), {"window_bits": 3}, mh.ERR_BAD_ARG, ""),
           ((fb2.base_words(b),), {"window_bits": 17}, mh.ERR_BAD_ARG, "")]
    for (base,), kw, code, word in bad:
        with pytest.raises(mh.MsmError) as e:
            ctx.fixed_base_g2_mul_device(base, d_k.data_ptr(), len(ks), d_xy.data_ptr(), d_inf.data_ptr(), **kw)
        assert e.value.code == code and word in str(e.value), (kw, str(e.value))
    with pytest.raises(mh.MsmError) as e:
        ctx.fixed_base_g2_mul(fb2.base_words(off), words)
    assert e.value.code == mh.ERR_INVALID_DATA and "subgroup" in str(e.value)
    with pytest.raises(mh.MsmError) as e:
        ctx.fixed_base_g2_mul_device(fb2.base_words(b), d_k.data_ptr(), 0, d_xy.data_ptr(), d_inf.data_ptr())
    assert e.value.code == mh.ERR_EMPTY
    with pytest.raises(mh.MsmError) as e:
        ctx.fixed_base_g2_mul(fb2.base_words(b), np.zeros((0, 8), np.uint32))
    assert e.value.code == mh.ERR_EMPTY
    for ptrs in ((d_k.data_ptr(), d_xy.data_ptr() + 4, d_inf.data_ptr()), (d_k.data_ptr() + 8, d_xy.data_ptr(), d_inf.data_ptr()),
                 (d_k.data_ptr(), d_xy.data_ptr(), d_inf.data_ptr() + 1), (None, d_xy.data_ptr(), d_inf.data_ptr()),
                 (d_k.data_ptr(), None, d_inf.data_ptr()), (d_k.data_ptr(), d_xy.data_ptr(), None)):
        with pytest.raises(mh.MsmError) as e:
            ctx.fixed_base_g2_mul_device(fb2.base_words(b), ptrs[0], len(ks), ptrs[1], ptrs[2])
        assert e.value.code == mh.ERR_BAD_ARG, ptrs
    got = host(d_xy, d_inf)
    assert (got[0] == FILL * 0x01010101).all() and (got[1] == FILL).all()  # no failed call wrote anything
    same(device_mul(ctx, fb2.base_words(a), words, window_bits=5), want_a, "a correct call after the errors: the old base's results")
    same(device_mul(ctx, fb2.base_words(GEN), ref[0][:100]), (ref[1][0][0][:100], ref[1][0][1][:100]), "and the default table again")


# 6
def test_two_streams(ctx, ref):
    import torch
    n = 2 * 64 * G + 1
    words = ref[0][:n]
    a = other_base()
    ks = [orc.words_to_int(w) for w in words[:40]]
    d_k = dev(words)
    xy1, inf1 = outputs(n)
    xy2, inf2 = outputs(40)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    ctx.fixed_base_g2_mul_device(fb2.base_words(GEN), d_k.data_ptr(), n, xy1.data_ptr(), inf1.data_ptr(), stream=s1.cuda_stream)
    ctx.fixed_base_g2_mul_device(fb2.base_words(a), d_k.data_ptr(), 40, xy2.data_ptr(), inf2.data_ptr(), stream=s2.cuda_stream)  # rebuilds the table
    ctx.fixed_base_g2_mul_device(fb2.base_words(a), d_k.data_ptr(), 40, xy2.data_ptr(), inf2.data_ptr(), flags=OS, stream=s1.cuda_stream)
    same(host(xy1, inf1), (ref[1][0][0][:n], ref[1][0][1][:n]), "stream 1")
    same(host(xy2, inf2), fb2.expected(ks, a, True), "stream 2, then stream 1 again")


# 7
def test_the_g1_and_g2_tables_coexist(ctx, ref):
    import torch
    n = 300
    words = ref[0][:n]
    ks = [orc.words_to_int(w) for w in words]
    want1 = fb.expected(ks)
    d_k = dev(words)
    for turn in range(3):
        xy1, inf1 = outputs(n, 16)
        xy2, inf2 = outputs(n)
        torch.cuda.synchronize()
        ctx.fixed_base_mul_device(fb.base_words(fb.GEN), d_k.data_ptr(), n, xy1.data_ptr(), inf1.data_ptr())
        ctx.fixed_base_g2_mul_device(fb2.base_words(GEN), d_k.data_ptr(), n, xy2.data_ptr(), inf2.data_ptr())
        same(host(xy1, inf1, 16), want1, ("G1", turn))
        same(host(xy2, inf2), (ref[1][0][0][:n], ref[1][0][1][:n]), ("G2", turn))


# 8
def test_scalars_to_g2_bases_to_msm_in_hbm(ctx):
    """k_i -> k_i * H as Montgomery words in HBM -> msm_bn254_g2_device with scalars s_i, one non-default stream, nothing crossing PCIe in between"""
    import torch
    n = 4096
    k, s = orc.gen_scalars(0xB2540031, n, nonzero=True), orc.gen_scalars(0xB2540032, n)
    k[5] = 0  # one identity among the bases: it travels as d_inf_mask
    d_k, d_s = dev(k), dev(s)
    d_xy, d_inf = outputs(n)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    ctx.fixed_base_g2_mul_device(fb2.base_words(GEN), d_k.data_ptr(), n, d_xy.data_ptr(), d_inf.data_ptr(), stream=st.cuda_stream)
    r = ctx.msm_g2_device(d_xy.data_ptr(), d_s.data_ptr(), n, d_inf.data_ptr(), stream=st.cuda_stream)
    total = sum(orc.words_to_int(a) * orc.words_to_int(b) for a, b in zip(k, s)) % R
    assert total and not r.is_infinity and r.affine_ints() == g2.mul(GEN, total)
    assert host(d_xy, d_inf)[1].sum() == 1
