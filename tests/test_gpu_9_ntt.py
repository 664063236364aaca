"""The BN254 scalar-field transforms on the GPU (-m gpu): msm_bn254_fr_ntt(_device) and msm_bn254_fr_mul_sub_scale_device against the
pure-Python yardstick (tools/bn254_fr_ntt_py.py), and the two Groth16 H recipes of INTEGRATION.md 4f end to end, into the resident MSM.
Inputs come from fixed seeds; every comparison is word-exact."""
import os
import random
import sys

import numpy as np
import pytest

import mopro_msm_hip as mh
from mopro_msm_hip import testhooks as th
from oracle import bn254_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bn254_fr_ntt_py as ny  # noqa: E402

pytestmark = pytest.mark.gpu
R = ny.R
INV, IM, OM = mh.NTT_INVERSE, mh.NTT_IN_MONT, mh.NTT_OUT_MONT
SMALL_TILE = 4


@pytest.fixture(scope="module")
def ctx():
    c = mh.MsmContext()
    yield c
    c.close()


@pytest.fixture(scope="module")
def hk():
    c = th.HooksContext()
    yield c
    c.close()


def words_of(vals):
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), "<u4").reshape(-1, 8).astype(np.uint32)


def ints_of(words):
    raw = np.ascontiguousarray(words, dtype=np.uint32).tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def rand_canonical(seed, n):
    """n canonical elements straight from numpy (top word < 0x30000000 < r's top word)"""
    g = np.random.default_rng(seed)
    w = g.integers(0, 1 << 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)
    w[:, 7] %= 0x30000000
    return w


def rand_vals(seed, n):
    rnd = random.Random(seed)
    return [rnd.randrange(R) for _ in range(n)]


def dev(words):
    import torch
    return torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint32).view(np.int32).copy()).to("cuda:0")


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32).reshape(-1, 8)


def device_ntt(c, words, log_n, batch=1, flags=0, coset=None):
    d = dev(words)
    c.ntt_device(d.data_ptr(), log_n, batch, flags, coset)
    return host(d)


@pytest.fixture(scope="module")
def forward_cases():
    """log_n -> (input words, the yardstick's forward transform), computed once"""
    out = {}
    for k in range(0, 15):
        w = words_of(rand_vals(0x9000 + k, 1 << k))
        out[k] = (w, ny.ntt_words(w, k))
    return out


# 1
@pytest.mark.parametrize("k", range(0, 15))
def test_forward_every_size_up_to_2_14(ctx, forward_cases, k):
    w, want = forward_cases[k]
    assert (device_ntt(ctx, w, k) == want).all()


# 2
@pytest.mark.parametrize("k", [1, 5, 11])
def test_flag_matrix(ctx, k):
    n = 1 << k
    x = rand_vals(0x9100 + k, 3 * n)
    std, mont = words_of(x), words_of([v * ny.MONT % R for v in x])
    for g in (None, 5, ny.root(k + 1)):
        for flags in range(8):
            inp = mont if flags & IM else std
            want = ny.ntt_words(inp, k, 3, flags, g)
            assert (device_ntt(ctx, inp, k, 3, flags, g) == want).all(), (k, g, flags)
            assert (device_ntt(ctx, inp[n:2 * n], k, 1, flags, g) == want[n:2 * n]).all(), (k, g, flags)
        for form in (0, IM | OM):  # inverse(forward(x)) == x, in either form
            inp = mont if form else std
            d = dev(inp)
            ctx.ntt_device(d.data_ptr(), k, 3, form, g)
            ctx.ntt_device(d.data_ptr(), k, 3, form | INV, g)
            assert (host(d) == inp).all(), (k, g, form)


# 3
def test_forced_small_tile(hk, forward_cases):
    want12 = device_ntt(hk, forward_cases[12][0], 12)
    assert (want12 == forward_cases[12][1]).all()
    hk.ntt_set_tile_log2(SMALL_TILE)
    try:
        for k in (4, 5, 8, 9, 12, 13):
            w, want = forward_cases[k]
            assert (device_ntt(hk, w, k) == want).all(), k
        k, g = 9, ny.root(10)
        x = words_of(rand_vals(0x9300, 3 << k))
        for flags in (INV | OM, IM, INV | IM | OM):
            assert (device_ntt(hk, x, k, 3, flags, g) == ny.ntt_words(x, k, 3, flags, g)).all(), flags
        with pytest.raises(mh.MsmError) as e:
            hk.ntt_set_tile_log2(7)
        assert e.value.code == mh.ERR_BAD_ARG
    finally:
        hk.ntt_set_tile_log2(0)
    assert (device_ntt(hk, forward_cases[12][0], 12) == want12).all()


# 4
def plan_boundaries():
    t = mh.ntt_plan(20)[0]
    return sorted({min(k, 22) for k in (t, t + 1, 2 * t, 2 * t + 1)})


@pytest.mark.parametrize("k", plan_boundaries())
def test_production_plan_boundaries(ctx, k):
    n = 1 << k
    if k <= 16:
        w = words_of(rand_vals(0x9400 + k, n))
        assert (device_ntt(ctx, w, k) == ny.ntt_words(w, k)).all()
        return
    # x[i] = c rho^i + 16 deltas: A[j] = c (rho^n - 1) / (rho w^j - 1) + sum_k c_k w^(j i_k)
    rnd = random.Random(0x9400 + k)
    c, rho = rnd.randrange(1, R), rnd.randrange(2, R)
    deltas = [(rnd.randrange(n), rnd.randrange(R)) for _ in range(16)]
    vals, p = [0] * n, c
    for i in range(n):
        vals[i] = p
        p = p * rho % R
    for i, v in deltas:
        vals[i] = (vals[i] + v) % R
    got = device_ntt(ctx, words_of(vals), k)
    w, top = ny.root(k), c * (pow(rho, n, R) - 1) % R
    js = [0, n - 1] + [rnd.randrange(n) for _ in range(512)]
    wj = [pow(w, j, R) for j in js]
    want = [(top * pow(rho * x - 1, R - 2, R) + sum(v * pow(x, i, R) for i, v in deltas)) % R for x in wj]
    assert ints_of(got[js]) == want
    x = rand_canonical(0x9480 + k, n)  # and a full round trip on a second, random array
    d = dev(x)
    ctx.ntt_device(d.data_ptr(), k)
    mid = host(d)
    assert not (mid == x).all()
    ctx.ntt_device(d.data_ptr(), k, 1, INV)
    assert (host(d) == x).all()


# 5
def test_words_at_or_above_r_are_read_modulo_r(ctx):
    k = 6
    rnd = random.Random(0x9500)
    vals = [rnd.randrange(R, 1 << 256) for _ in range(1 << k)]
    vals[0], vals[1], vals[2] = (1 << 256) - 1, R, R + 1
    w, reduced = words_of(vals), words_of([v % R for v in vals])
    for flags, g in ((0, None), (INV, None), (OM, 5), (INV, ny.root(k + 1))):
        got = device_ntt(ctx, w, k, 1, flags, g)
        assert (got == ny.ntt_words(w, k, 1, flags, g)).all() and (got == device_ntt(ctx, reduced, k, 1, flags, g)).all(), (flags, g)
    assert (device_ntt(ctx, w[:1], 0) == reduced[:1]).all()  # log_n == 0: form conversion only


# 6
def test_host_call_matches_device_call(ctx):
    for k, batch, flags, g in ((7, 1, 0, None), (11, 3, INV | OM, 5), (15, 1, IM, ny.root(16))):  # (2^15 x 32 B = 1 MiB: pinned in place)
        w = rand_canonical(0x9600 + k, batch << k)
        want = device_ntt(ctx, w, k, batch, flags, g)
        keep = w.copy()
        assert (ctx.ntt(w, k, batch, flags, g) == want).all() and (w == keep).all()
        assert ctx.ntt(w, k, batch, flags, g, out=w) is not None and (w == want).all()  # out == in


# 7
def test_groth16_h_recipes_end_to_end(ctx):
    import torch
    k = 10
    n = 1 << k
    a, b = rand_vals(0x9701, n), rand_vals(0x9702, n)
    c = [x * y % R for x, y in zip(a, b)]
    abc = words_of(a + b + c)
    st = torch.cuda.Stream(device="cuda:0")
    s = st.cuda_stream

    def on_stream(g, kscale, last_flags):
        d = dev(abc)
        torch.cuda.synchronize()
        p = d.data_ptr()
        ctx.ntt_device(p, k, 3, INV | OM, None, s)                      # evaluations -> coefficients, kept as Montgomery words
        ctx.ntt_device(p, k, 3, IM | OM, g, s)                          # coefficients -> evaluations on the coset
        ctx.fr_mul_sub_scale_device(p, p + 32 * n, p + 64 * n, p, n, kscale, last_flags, s)  # into a's place
        return d

    # arkworks LibsnarkReduction: g = 5, divide by Z(g w^j) = 5^n - 1, back to coefficients: standard form for the MSM
    zinv = pow(pow(5, n, R) - 1, R - 2, R)
    d = on_stream(5, zinv, IM | OM)
    ctx.ntt_device(d.data_ptr(), k, 1, INV | IM, 5, s)
    pa, pb, pc = (ny.ntt(v, 1, True) for v in (a, b, c))
    ea, eb, ec = (ny.ntt(v, 5) for v in (pa, pb, pc))
    h = ny.ntt([(x * y - z) * zinv % R for x, y, z in zip(ea, eb, ec)], 5, True)
    assert h[n - 1] == 0 and any(h)
    logs = orc.gen_scalars(0x9703, n, nonzero=True)
    bases = orc.gen_bases_from_logs(logs, orc.FORM_MONT)
    ctx.upload_bases(bases, mh.FORM_MONT)
    r = ctx.msm_resident_device(d.data_ptr(), n, s)  # h never left HBM
    st.synchronize()
    assert (host(d)[:n] == words_of(h)).all()
    exp, einf, _ = orc.msm_pippenger(bases, words_of(h), orc.FORM_MONT)
    assert bool(r.is_infinity) == bool(einf) and (r.affine_std == exp).all()

    # snarkjs: the odd coset g = w_(k+1), no division: (A B - C)(g w^j) = h(g w^j) * (g^n - 1) = -2 h(g w^j)
    g = ny.root(k + 1)
    d = on_stream(g, None, IM)
    st.synchronize()
    ea, eb, ec = (ny.ntt(v, g) for v in (pa, pb, pc))
    want = [(x * y - z) % R for x, y, z in zip(ea, eb, ec)]
    assert (host(d)[:n] == words_of(want)).all()
    assert want == [(R - 2) * v % R for v in ny.ntt(h, g)]


# 8
@pytest.mark.parametrize("n", [1, 255, 1000])
def test_mul_sub_scale(ctx, n):
    rnd = random.Random(0x9800 + n)
    vals = lambda: words_of([rnd.randrange(1 << 256) if i % 5 == 0 else rnd.randrange(R) for i in range(n)])
    a, b, c = vals(), vals(), vals()
    kk = rnd.randrange(1, R)
    for flags in (0, IM, OM, IM | OM):
        for use_c, k in ((True, kk), (False, kk), (True, None), (False, None)):
            da, db, dc, do = dev(a), dev(b), dev(c), dev(np.zeros_like(a))
            want = ny.mul_sub_scale_words(a, b, c if use_c else None, k, flags)
            ctx.fr_mul_sub_scale_device(da.data_ptr(), db.data_ptr(), dc.data_ptr() if use_c else None, do.data_ptr(), n, k, flags)
            assert (host(do) == want).all(), (flags, use_c, k)
            ctx.fr_mul_sub_scale_device(da.data_ptr(), db.data_ptr(), dc.data_ptr() if use_c else None, da.data_ptr(), n, k, flags)  # out aliases a
            assert (host(da) == want).all() and (host(db) == b).all(), (flags, use_c, k)


# 9
def test_errors_leave_the_context_usable(ctx, forward_cases):
    w, want = forward_cases[6]

    def good():
        assert (device_ntt(ctx, w, 6) == want).all()

    d = dev(w)
    p = d.data_ptr()
    for call, code in ((lambda: ctx.ntt_device(p, 29), mh.ERR_BAD_ARG),
                       (lambda: ctx.ntt_device(p, 6, 0), mh.ERR_EMPTY),
                       (lambda: ctx.ntt_device(None, 6), mh.ERR_BAD_ARG),
                       (lambda: ctx.ntt_device(p, 6, 1, 8), mh.ERR_BAD_ARG),
                       (lambda: ctx.ntt_device(p, 6, 1, 0, 0), mh.ERR_BAD_ARG),
                       (lambda: ctx.ntt_device(p, 6, 1, INV, R), mh.ERR_BAD_ARG),
                       (lambda: ctx.fr_mul_sub_scale_device(p, p, None, p, 0), mh.ERR_EMPTY),
                       (lambda: ctx.fr_mul_sub_scale_device(p, None, None, p, 4), mh.ERR_BAD_ARG),
                       (lambda: ctx.fr_mul_sub_scale_device(p, p, None, p, 4, None, INV), mh.ERR_BAD_ARG)):
        with pytest.raises(mh.MsmError) as e:
            call()
        assert e.value.code == code
        good()
    assert (host(d) == w).all()  # no failed call touched the array
    lib = ctx._lib  # the host-pointer call, NULL out
    assert lib.msm_bn254_fr_ntt(ctx._h, w.ctypes.data_as(mh._u32p), None, 6, 1, 0, None) == mh.ERR_BAD_ARG
    good()


# 10
def test_tables_are_reused_and_equal_across_contexts(forward_cases):
    seen = []
    for _ in range(2):
        with mh.MsmContext() as c:
            got = [device_ntt(c, forward_cases[k][0], k) for k in (12, 8, 12)]
            got += [device_ntt(c, forward_cases[12][0], 12, 1, INV, 5), device_ntt(c, forward_cases[8][0], 8, 1, 0, 5),
                    device_ntt(c, forward_cases[12][0], 12, 1, INV, 5)]
            seen.append(got)
    for got in seen:
        assert (got[0] == forward_cases[12][1]).all() and (got[1] == forward_cases[8][1]).all() and (got[2] == got[0]).all()
        assert (got[3] == ny.ntt_words(forward_cases[12][0], 12, 1, INV, 5)).all() and (got[5] == got[3]).all()
    assert all((x == y).all() for x, y in zip(*seen))
