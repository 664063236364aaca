"""The scalar-field scans on the GPU (-m gpu): msm_bn254_fr_poly_eval_device, _poly_div_linear(_device) and _running_product_device against the
Python yardstick of tools/bn254_fr_scan_py.py (Python integers, never the library) -- sizes around a chain, a wavefront's range and a workgroup,
and with the hooks library's chain of one element the sizes at which the launch over the workgroups' aggregates takes a second round; the
classes of points and coefficient sets, zeros at every place of the product, the flag matrix, aliasing, errors and state, two streams; the
existing calls (powers, lincomb, batch inverse, mul_sub_scale) as a second witness without the yardstick; and a KZG commitment and opening end
to end on one stream, checked by the CPU oracle.  Inputs come from fixed seeds; every comparison is word-exact; every output array is
pre-filled and has guard elements behind it that must keep the fill."""
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
import bn254_fr_scan_py as fs  # noqa: E402
import fixed_base_cases as fb  # noqa: E402

pytestmark = pytest.mark.gpu
R = fs.R
IM, OM, EX = mh.NTT_IN_MONT, mh.NTT_OUT_MONT, mh.FR_SCAN_EXCLUSIVE
FLAG_SETS = (0, IM, OM, IM | OM)
FILL = 0x5A5A5A5A  # every output word before a call: an element the kernels skip shows up, and so does one written past n
GUARD = 4  # elements behind every output array that must keep the fill
PLAN = mh.fr_scan_plan(1)  # (host only)
G, B = PLAN["chain"], PLAN["block_points"]
SIZES = sorted({n for n in (1, 2, G - 1, G, G + 1, 64 * G - 1, 64 * G, 64 * G + 1, B - 1, B, B + 1, 2 * B + 1, 3 * B - 1) if n >= 1})
TWO_ROUNDS = (256 * 256 + 3, 2 * 256 * 256 - 1)  # with a chain of one element: 257 and 512 workgroups
SETS = ("zero", "r-1", "ones", "random", "multiple", "monomial")


@pytest.fixture(scope="module")
def ctx():
    c = mh.MsmContext()
    yield c
    c.close()


@pytest.fixture(scope="module")
def hk():
    c = th.HooksContext()
    c.fr_scan_set_chain(1)
    yield c
    c.close()


def dev(words):
    import torch
    return torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint32).view(np.int32).copy()).to("cuda:0")


def filled(n, words=None):
    """n + GUARD elements of fill; the first n are `words` when given"""
    a = np.full((n + GUARD, 8), FILL, np.uint32)
    if words is not None:
        a[:n] = words
    return dev(a)


def host(t, n=None):
    """the first n elements of an array made by filled(n); the guard behind them must be untouched"""
    import torch
    torch.cuda.synchronize()
    a = t.cpu().numpy().view(np.uint32).reshape(-1, 8)
    if n is None:
        return a
    assert (a[n:] == FILL).all(), "written past n"
    return a[:n]


def same(got, want, what=None):
    assert got.shape == want.shape, what
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (what, "first wrong element", int(bad[0]), "of", got.shape[0], "wrong", int(bad.size))


def sync():
    import torch
    torch.cuda.synchronize()  # the arrays were made on torch's stream


def divide(c, coeffs, z, flags=0, inplace=False, rem=True):
    """(quotient words, remainder words or None) of one device call on the patterns `coeffs`"""
    n = len(coeffs)
    w = fs.to_words(coeffs)
    d_in, d_rem = filled(n, w), filled(1)
    d_out = d_in if inplace else filled(n)
    sync()
    c.fr_poly_div_linear_device(d_in.data_ptr(), n, z, d_out.data_ptr(), d_rem.data_ptr() if rem else None, flags)
    q = host(d_out, n)
    if not inplace:
        assert (host(d_in, n) == w).all()
    if not rem:
        assert (host(d_rem) == FILL).all()
    return q, host(d_rem, 1) if rem else None


def evaluate(c, coeffs, z, flags=0):
    n = len(coeffs)
    d_in, d_val = dev(fs.to_words(coeffs)), filled(1)
    sync()
    c.fr_poly_eval_device(d_in.data_ptr(), n, z, d_val.data_ptr(), flags)
    return host(d_val, 1)


def product(c, xs, flags=0, inplace=False, total=True):
    n = len(xs)
    w = fs.to_words(xs)
    d_in, d_tot = filled(n, w), filled(1)
    d_out = d_in if inplace else filled(n)
    sync()
    c.fr_running_product_device(d_in.data_ptr(), d_out.data_ptr(), n, d_tot.data_ptr() if total else None, flags)
    out = host(d_out, n)
    if not inplace:
        assert (host(d_in, n) == w).all()
    if not total:
        assert (host(d_tot) == FILL).all()
    return out, host(d_tot, 1) if total else None


def check_division(c, coeffs, z, flags=0, inplace=False, what=None):
    q, rem = fs.poly_div_linear(fs.read(coeffs, bool(flags & IM)), z)
    got_q, got_rem = divide(c, coeffs, z, flags, inplace)
    same(got_q, fs.write(q, bool(flags & OM)), what)
    same(got_rem, fs.write([rem], bool(flags & OM)), (what, "remainder"))
    same(evaluate(c, coeffs, z, flags), got_rem, (what, "poly_eval equals the remainder"))
    return q, rem


def check_product(c, xs, flags=0, inplace=False, total=True, what=None):
    out, tot = fs.running_product(fs.read(xs, bool(flags & IM)), bool(flags & EX))
    got, got_tot = product(c, xs, flags, inplace, total)
    same(got, fs.write(out, bool(flags & OM)), what)
    if total:
        same(got_tot, fs.write([tot], bool(flags & OM)), (what, "total"))


# 1
@pytest.mark.parametrize("n", SIZES)
def test_division_sizes_points_and_coefficient_sets(ctx, n):
    """every size with every coefficient set; the point moves through its six classes with the set and the size, so every set meets every point"""
    si = SIZES.index(n)
    zs = fs.points(0x2500 + n)
    for ci, name in enumerate(SETS):
        z = zs[(si + ci) % 6]
        coeffs = fs.coefficient_sets(0x2510 + n, n, z)[name]
        q, rem = check_division(ctx, coeffs, z, inplace=bool((si + ci) & 1), what=(n, name, hex(z)))
        if name == "multiple" and n > 1:
            assert rem == 0 and q[:-1] == [v % R for v in fs.patterns(0x2511 + n, n - 1)]  # p = (X - z) s: q == s


# 2
@pytest.mark.parametrize("zi", range(6))
def test_division_every_point_with_every_set(ctx, zi):
    n = 64 * G + 1
    z = fs.points(0x2520)[zi]
    for name in SETS:
        check_division(ctx, fs.coefficient_sets(0x2521, n, z)[name], z, what=(name, hex(z)))
    q, rem = divide(ctx, [5, 6, 7], 0)  # z = 0: the shift
    assert fs.from_words(q) == [6, 7, 0] and fs.from_words(rem) == [5]
    q, rem = divide(ctx, [R + 9], fs.points(0)[zi])  # n = 1
    assert fs.from_words(q) == [0] and fs.from_words(rem) == [9]


# 3
@pytest.mark.parametrize("n", [G + 1, 64 * G + 1, B + 1, 2 * B + 1])
def test_flag_matrix(ctx, n):
    z = fs.points(0x2530 + n)[5]
    xs = fs.product_sets(0x2531 + n, n)["random"]
    xs[:5] = [(1 << 256) - 1, R - 1, R + 1, 2 * R + 3, 1]
    for flags in FLAG_SETS:
        for name in ("random", "multiple"):
            check_division(ctx, fs.coefficient_sets(0x2532 + n, n, z, bool(flags & IM))[name], z, flags, what=(n, name, flags))
        for ex in (0, EX):
            check_product(ctx, xs, flags | ex, what=(n, flags, ex))


# 4
@pytest.mark.parametrize("n", SIZES)
def test_product_sizes_modes_and_total(ctx, n):
    si = SIZES.index(n)
    sets = fs.product_sets(0x2540 + n, n, (0, n // 2, n - 1))
    for ci, name in enumerate(sorted(sets)):
        for ex in (0, EX):
            check_product(ctx, sets[name], ex, inplace=bool((si + ci) & 1), total=bool((si + ci + (ex >> 5)) & 1) or name == "random", what=(n, name, ex))


# 5
def test_a_zero_zeroes_what_follows_and_nothing_before(ctx):
    """the first, middle and last place of a chain, of a wavefront's range and of a block, all in the second block"""
    n = 2 * B + 1
    chain, wave = B + 5 * G, B + 64 * G
    places = sorted({chain, chain + G // 2, chain + G - 1, wave, wave + 32 * G, wave + 64 * G - 1, B, B + B // 2, 2 * B - 1})
    sets = fs.product_sets(0x2550, n, places)
    clean, _ = product(ctx, sets["random"])
    for at in places:
        for flags in (0, EX):
            got, tot = product(ctx, sets["zero@%d" % at], flags)
            cut = at + (flags >> 5)  # exclusive: the zero shows one place later
            ref = clean if not flags else np.concatenate([fs.write([1]), clean[:-1]])
            assert (got[:cut] == ref[:cut]).all() and not got[cut:].any() and got[cut - 1].any() and not tot.any(), (at, flags)
        check_product(ctx, sets["zero@%d" % at], what=at)


# 6
def test_in_place_equals_out_of_place(ctx, hk):
    for c, sizes in ((ctx, (B + 1, 2 * B + 1)), (hk, (TWO_ROUNDS[0],))):
        for n in sizes:
            z = fs.points(0x2560 + n)[5]
            coeffs = fs.patterns(0x2561 + n, n)
            q0, r0 = divide(c, coeffs, z, IM)
            q1, r1 = divide(c, coeffs, z, IM, inplace=True)
            same(q1, q0, (n, "d_quot == d_coeffs"))
            same(r1, r0, n)
            for ex in (0, EX):
                o0, t0 = product(c, coeffs, OM | ex)
                o1, t1 = product(c, coeffs, OM | ex, inplace=True)
                same(o1, o0, (n, ex, "d_out == d_in"))
                same(t1, t0, n)


# 7
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 513, 767, *TWO_ROUNDS])
def test_a_chain_of_one_element(hk, n):
    """the hooks library with msm_test_fr_scan_set_chain(1): a workgroup covers 256 elements, and from 2^16 + 1 elements on the launch over the
    aggregates walks them in more than one round"""
    assert mh.fr_scan_plan(n)["chain"] == G  # (the plan is the product's)
    z = fs.points(0x2570 + n)[5 if n > 767 else n % 6]
    big = n > 767
    for name in ("random", "multiple") if big else SETS:
        check_division(hk, fs.coefficient_sets(0x2571 + n, n, z)[name], z, inplace=bool(n & 1), what=(n, name))
    sets = fs.product_sets(0x2572 + n, n, (n // 2,) if big else (0, n // 2, n - 1))
    for name in sorted(sets):
        if not (big and name == "one"):
            check_product(hk, sets[name], EX if n & 2 else 0, inplace=bool(n & 1), what=(n, name))
    if big:
        check_product(hk, sets["random"], 0 if n & 2 else EX, what=(n, "the other mode"))


def test_the_setter_takes_its_two_chains_only(hk):
    for chain in (2, 7, 16):
        with pytest.raises(mh.MsmError) as e:
            hk.fr_scan_set_chain(chain)
        assert e.value.code == mh.ERR_BAD_ARG
    coeffs = fs.patterns(0x2580, 3 * B - 1)
    z = fs.points(0x2580)[5]
    q1, r1 = divide(hk, coeffs, z)
    hk.fr_scan_set_chain(0)
    try:
        q8, r8 = divide(hk, coeffs, z)
        hk.fr_scan_set_chain(8)
        q8b, _ = divide(hk, coeffs, z)
    finally:
        hk.fr_scan_set_chain(1)
    same(q8, q1, "both chains")
    same(q8b, q1)
    same(r8, r1)


# 8: against existing calls, without the yardstick
def test_the_monomial_against_the_powers(ctx):
    for n in (2, 64 * G + 1, 2 * B + 1):
        z = fs.patterns(0x2590 + n, 1)[0]
        q, rem = divide(ctx, [0] * (n - 1) + [1], z)
        d_pow = filled(n)
        sync()
        ctx.fr_powers_device(z, d_pow.data_ptr(), n)
        pw = host(d_pow, n)
        same(q[:n - 1], pw[:n - 1][::-1], (n, "q[j] = z^(n - 2 - j)"))  # reversed on the host
        assert not q[n - 1].any()
        same(rem, pw[n - 1:], (n, "p(z) = z^(n - 1)"))


def test_the_quotient_times_the_divisor_by_lincomb(ctx):
    """q[j - 1] - z q[j] reproduces p[j], j = 1 .. n - 1: one msm_bn254_fr_lincomb_device over n - 1 elements"""
    for n in (2, B + 1, 3 * B - 1):
        z = fs.patterns(0x25A0 + n, 1)[0]
        coeffs = [v % R for v in fs.patterns(0x25A1 + n, n)]
        d_p, d_q, d_back = dev(fs.to_words(coeffs)), filled(n), filled(n - 1)
        sync()
        ctx.fr_poly_div_linear_device(d_p.data_ptr(), n, z, d_q.data_ptr())
        ctx.fr_lincomb_device(d_q.data_ptr(), d_back.data_ptr(), n - 1, 1, d_q.data_ptr() + 32, (R - z % R) % R)
        same(host(d_back, n - 1), fs.to_words(coeffs[1:]), n)
        host(d_q, n)


def test_the_product_of_a_constant_against_the_powers(ctx):
    n = 2 * B + 1
    b = fs.patterns(0x25B0, 1)[0]
    d_in, d_out, d_pow = dev(fs.to_words([b] * n)), filled(n), filled(n)
    sync()
    ctx.fr_running_product_device(d_in.data_ptr(), d_out.data_ptr(), n)
    ctx.fr_powers_device(b, d_pow.data_ptr(), n, first=1)
    same(host(d_out, n), host(d_pow, n), "b^(i + 1)")


def test_the_grand_product_of_a_permutation_is_one(ctx):
    """Z from f and a permutation g of it: batch_inverse(g) -> mul_sub_scale(f, 1 / g) -> exclusive product: the total is 1"""
    n = 2 * B + 1
    f = [x if x % R else 1 for x in fs.patterns(0x25C0, n)]
    g = list(f)
    random.Random(0x25C1).shuffle(g)
    d_f, d_g, d_t, d_z, d_tot = dev(fs.to_words(f)), dev(fs.to_words(g)), filled(n), filled(n), filled(1)
    sync()
    ctx.fr_batch_inverse_device(d_g.data_ptr(), d_g.data_ptr(), n)
    ctx.fr_mul_sub_scale_device(d_f.data_ptr(), d_g.data_ptr(), None, d_t.data_ptr(), n)
    ctx.fr_running_product_device(d_t.data_ptr(), d_z.data_ptr(), n, d_tot.data_ptr(), EX)
    assert fs.from_words(host(d_tot, 1)) == [1]
    z = fs.from_words(host(d_z, n))
    assert z[0] == 1 and all(z[i + 1] * (g[i] % R) % R == z[i] * (f[i] % R) % R for i in range(n - 1))
    host(d_t, n)


# 9
def test_host_form_equals_device_form(ctx):
    for n, flags in ((1, 0), (64 * G + 1, IM), (B + 1, OM), (3 * B - 1, IM | OM)):
        coeffs = fs.patterns(0x25D0 + n, n)
        z = fs.points(0x25D1 + n)[n % 6]
        q, rem = ctx.fr_poly_div_linear(fs.to_words(coeffs), z, flags)
        dq, drem = divide(ctx, coeffs, z, flags)
        same(q, dq, (n, flags))
        same(rem.reshape(1, 8), drem, (n, flags))
    a = fs.to_words(fs.patterns(0x25D2, 300))
    want, _ = ctx.fr_poly_div_linear(a, 77)
    q, _ = ctx.fr_poly_div_linear(a, 77, out=a)  # quot == coeffs
    assert q is not None and (a == want).all()
    lib, h = mh.load_library(), ctx._h
    import ctypes as C
    p32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint32))
    b, out, zw = fs.to_words(fs.patterns(0x25D2, 300)), np.zeros((300, 8), np.uint32), fs.to_words([77])
    assert lib.msm_bn254_fr_poly_div_linear(h, p32(b), 300, p32(zw), p32(out), None, 0) == mh.OK and (out == want).all()  # rem NULL


# 10
def errors(c, p_in, p_out, p_one, n):
    z = 3
    BA, EM = mh.ERR_BAD_ARG, mh.ERR_EMPTY
    return [(lambda: c.fr_poly_eval_device(None, n, z, p_one), BA), (lambda: c.fr_poly_eval_device(p_in, n, None, p_one), BA),
            (lambda: c.fr_poly_eval_device(p_in, n, z, None), BA), (lambda: c.fr_poly_eval_device(p_in + 4, n, z, p_one), BA),
            (lambda: c.fr_poly_eval_device(p_in, n, z, p_one + 8), BA), (lambda: c.fr_poly_eval_device(p_in, n, z, p_one, 1), BA),
            (lambda: c.fr_poly_eval_device(p_in, n, z, p_one, EX), BA), (lambda: c.fr_poly_eval_device(p_in, 0, z, p_one), EM),
            (lambda: c.fr_poly_eval_device(p_in, (1 << 36) + 1, z, p_one), BA),
            (lambda: c.fr_poly_div_linear_device(None, n, z, p_out), BA), (lambda: c.fr_poly_div_linear_device(p_in, n, None, p_out), BA),
            (lambda: c.fr_poly_div_linear_device(p_in, n, z, None), BA), (lambda: c.fr_poly_div_linear_device(p_in + 4, n, z, p_out), BA),
            (lambda: c.fr_poly_div_linear_device(p_in, n, z, p_out + 8), BA), (lambda: c.fr_poly_div_linear_device(p_in, n, z, p_out, p_one + 12), BA),
            (lambda: c.fr_poly_div_linear_device(p_in, n, z, p_out, p_one, 8), BA), (lambda: c.fr_poly_div_linear_device(p_in, n, z, p_out, p_one, EX), BA),
            (lambda: c.fr_poly_div_linear_device(p_in, 0, z, p_out), EM), (lambda: c.fr_poly_div_linear_device(p_in, (1 << 36) + 1, z, p_out), BA),
            (lambda: c.fr_poly_div_linear(np.zeros((0, 8), np.uint32), z), EM), (lambda: c.fr_poly_div_linear(np.zeros((5, 8), np.uint32), z, 16), BA),
            (lambda: c.fr_poly_div_linear(np.zeros((5, 8), np.uint32), None), BA),
            (lambda: c.fr_running_product_device(None, p_out, n), BA), (lambda: c.fr_running_product_device(p_in, None, n), BA),
            (lambda: c.fr_running_product_device(p_in + 4, p_out, n), BA), (lambda: c.fr_running_product_device(p_in, p_out + 8, n), BA),
            (lambda: c.fr_running_product_device(p_in, p_out, n, p_one + 4), BA), (lambda: c.fr_running_product_device(p_in, p_out, n, p_one, 1), BA),
            (lambda: c.fr_running_product_device(p_in, p_out, n, p_one, 64), BA), (lambda: c.fr_running_product_device(p_in, p_out, 0), EM),
            (lambda: c.fr_running_product_device(p_in, p_out, (1 << 36) + 1), BA)]


def test_errors_leave_the_outputs_and_the_context_alone():
    """every error case on a FRESH context (the first call it ever sees is a refused one), then a correct call; and a first correct call on another"""
    n = B + 5
    coeffs = fs.patterns(0x25E0, n)
    q, rem = fs.poly_div_linear(fs.read(coeffs), 3)
    with mh.MsmContext() as c:
        d_in, d_out, d_one = dev(fs.to_words(coeffs)), filled(n), filled(1)
        sync()
        for i, (call, code) in enumerate(errors(c, d_in.data_ptr(), d_out.data_ptr(), d_one.data_ptr(), n)):
            with pytest.raises(mh.MsmError) as e:
                call()
            assert e.value.code == code, (i, str(e.value))
        assert (host(d_out) == FILL).all() and (host(d_one) == FILL).all()  # no failed call wrote anything
        c.fr_poly_div_linear_device(d_in.data_ptr(), n, 3, d_out.data_ptr(), d_one.data_ptr())
        same(host(d_out, n), fs.write(q), "a correct call after the errors")
        same(host(d_one, 1), fs.write([rem]))
        with pytest.raises(mh.MsmError):
            c.fr_running_product_device(d_in.data_ptr(), d_out.data_ptr(), n, flags=8)
        c.fr_running_product_device(d_in.data_ptr(), d_out.data_ptr(), n, d_one.data_ptr(), EX)
        out, tot = fs.running_product(fs.read(coeffs), True)
        same(host(d_out, n), fs.write(out), "and another, of the other kind")
        same(host(d_one, 1), fs.write([tot]))
    for first in ("eval", "product", "host"):  # a first call on a fresh context
        with mh.MsmContext() as c:
            if first == "eval":
                same(evaluate(c, coeffs, 3), fs.write([rem]), first)
            elif first == "product":
                check_product(c, coeffs, what=first)
            else:
                got_q, got_rem = c.fr_poly_div_linear(fs.to_words(coeffs), 3)
                same(got_q, fs.write(q), first)
                assert fs.from_words(got_rem) == [rem]


# 11
def test_two_streams(ctx):
    """calls interleaved on two streams of one context share the context's array of aggregates: the event behind each call orders them"""
    import torch
    n = 3 * B - 1
    a, b = fs.patterns(0x25F0, n), [x if x % R else 1 for x in fs.patterns(0x25F1, n)]
    za, zb = fs.patterns(0x25F2, 2)
    d_a, d_b = dev(fs.to_words(a)), dev(fs.to_words(b))
    d_qa, d_ra, d_pb, d_tb, d_qb, d_va = filled(n), filled(1), filled(n), filled(1), filled(n), filled(1)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    sync()
    for _ in range(3):
        ctx.fr_poly_div_linear_device(d_a.data_ptr(), n, za, d_qa.data_ptr(), d_ra.data_ptr(), stream=s1.cuda_stream)
        ctx.fr_running_product_device(d_b.data_ptr(), d_pb.data_ptr(), n, d_tb.data_ptr(), stream=s2.cuda_stream)
        ctx.fr_poly_eval_device(d_a.data_ptr(), n, za, d_va.data_ptr(), stream=s1.cuda_stream)
        ctx.fr_poly_div_linear_device(d_b.data_ptr(), n, zb, d_qb.data_ptr(), stream=s2.cuda_stream)
    qa, ra = fs.poly_div_linear(fs.read(a), za)
    qb, _ = fs.poly_div_linear(fs.read(b), zb)
    pb, tb = fs.running_product(fs.read(b))
    same(host(d_qa, n), fs.write(qa), "stream 1: division")
    same(host(d_ra, 1), fs.write([ra]), "stream 1: remainder")
    same(host(d_va, 1), fs.write([ra]), "stream 1: evaluation")
    same(host(d_pb, n), fs.write(pb), "stream 2: product")
    same(host(d_tb, 1), fs.write([tb]), "stream 2: total")
    same(host(d_qb, n), fs.write(qb), "stream 2: division")


# 12
def oracle_mul(xy_std_words, k):
    return orc.g1_scalar_mul(np.ascontiguousarray(xy_std_words, np.uint32), orc.int_to_words(k % R))


def affine(jac):
    xy, inf = orc.g1_to_affine_std(jac)
    return None if inf else (orc.words_to_int(xy[:8]), orc.words_to_int(xy[8:]))


@pytest.mark.parametrize("degree_gap", [0, 37])
def test_kzg_commit_and_open_on_one_stream(ctx, degree_gap):
    """powers of tau -> fixed-base points (the SRS) -> C = MSM(p) -> q, y = p / (X - z) -> pi = MSM(q), all on one non-default stream; the CPU
    oracle checks C = p(tau) G, pi = q(tau) G and C - y G = (tau - z) pi.  Once more with 2^12 - 37 coefficients zero-padded to the SRS"""
    import torch
    n = 1 << 12
    rnd = random.Random(0x2600 + degree_gap)
    tau, z = rnd.randrange(1, R), rnd.getrandbits(256)
    p = [rnd.randrange(R) for _ in range(n - degree_gap)] + [0] * degree_gap  # (canonical: the MSM refuses scalars >= 2^254)
    d_tau, d_srs = filled(n), dev(np.full((n + GUARD, 16), FILL, np.uint32))
    d_inf = torch.full((n + GUARD,), 0x5A, dtype=torch.uint8, device="cuda:0")
    d_p, d_q, d_y = dev(fs.to_words(p)), filled(n), filled(1)
    st = torch.cuda.Stream()
    s = st.cuda_stream
    sync()
    ctx.fr_powers_device(tau, d_tau.data_ptr(), n, stream=s)
    ctx.fixed_base_mul_device(fb.base_words(fb.GEN), d_tau.data_ptr(), n, d_srs.data_ptr(), d_inf.data_ptr(), stream=s)
    commit = ctx.msm_device(d_srs.data_ptr(), d_p.data_ptr(), n, d_inf.data_ptr(), stream=s)
    ctx.fr_poly_div_linear_device(d_p.data_ptr(), n, z, d_q.data_ptr(), d_y.data_ptr(), stream=s)
    proof = ctx.msm_device(d_srs.data_ptr(), d_q.data_ptr(), n, d_inf.data_ptr(), stream=s)
    st.synchronize()
    q, y = fs.poly_div_linear(fs.read(p), z)
    same(host(d_q, n), fs.write(q), "the quotient")
    assert fs.from_words(host(d_y, 1)) == [y]
    assert (d_inf.cpu().numpy()[n:] == 0x5A).all() and not d_inf.cpu().numpy()[:n].any()
    assert commit.affine_ints() == fb.point(fs.poly_eval(fs.read(p), tau)) and commit.affine_ints() is not None  # C = p(tau) G
    assert proof.affine_ints() == fb.point(fs.poly_eval(q, tau)) and proof.affine_ints() is not None            # pi = q(tau) G
    gen = fb.base_words(fb.GEN)
    lhs = affine(orc.g1_add(oracle_mul(commit.affine_std, 1), oracle_mul(gen, R - y)))
    rhs = affine(oracle_mul(proof.affine_std, tau - z))
    assert lhs == rhs and lhs is not None  # C - y G = (tau - z) pi
