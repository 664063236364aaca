"""The scalar vectors of a setup on the GPU (-m gpu): msm_bn254_fr_powers_device, _batch_inverse(_device), _lagrange_device and _lincomb_device
against the Python yardstick of tools/bn254_fr_vectors_py.py (Python integers, never the library) -- sizes around a chain, a wave of chains and a
workgroup, zeros at every place of a chain, the flag matrix, aliasing, errors, two streams; the adjoint check that ties the Lagrange vector and
the transposed matrices to the existing row evaluation without the yardstick; and Lagrange -> transposed rows -> lincomb / powers -> fixed-base
points end to end on one stream.  Inputs come from fixed seeds; every comparison is word-exact."""
import json
import os
import random
import sys

import numpy as np
import pytest

import mopro_msm_hip as mh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bn254_fr_vectors_py as frv  # noqa: E402
import fixed_base_cases as fb  # noqa: E402
import fixed_base_g2_cases as fb2  # noqa: E402

pytestmark = pytest.mark.gpu
R = frv.R
IM, OM = mh.NTT_IN_MONT, mh.NTT_OUT_MONT
FLAG_SETS = (0, IM, OM, IM | OM)
FILL = 0x5A5A5A5A  # every output word before a call: an element the kernels skip shows up, and so does one written past n
PLAN = mh.fr_vector_plan()  # (host only)
G, B, PB = PLAN["inv_group"], PLAN["block_points"], PLAN["powers_block_points"]
BIG = (1 << 14) + 5
SIZES = sorted({1, 2, 63, 64, 65, 64 * G - 1, 64 * G, 64 * G + 1, B - 1, B + 1, BIG})
GUARD = 4  # elements behind every output array that must keep the fill


@pytest.fixture(scope="module")
def ctx():
    c = mh.MsmContext()
    yield c
    c.close()


def dev(words):
    import torch
    return torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint32).view(np.int32).copy()).to("cuda:0")


def filled(n):
    return dev(np.full((n + GUARD, 8), FILL, np.uint32))


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


@pytest.fixture(scope="module")
def ref():
    """BIG seeded 256-bit patterns (most of them >= r) and the inverses of what they spell, per input form, computed once; the tests take
    prefixes"""
    pats = [p if p % R else 1 for p in frv.patterns(0xF5EC, BIG)]
    return pats, frv.to_words(pats), {m: frv.batch_inverse(frv.read(pats, m)) for m in (False, True)}


# 1
@pytest.mark.parametrize("n", SIZES)
def test_batch_inverse_sizes_and_flags(ctx, ref, n):
    pats, words, inv = ref
    for flags in FLAG_SETS:
        d_in, d_out = dev(words[:n]), filled(n)
        sync()
        ctx.fr_batch_inverse_device(d_in.data_ptr(), d_out.data_ptr(), n, flags)
        same(host(d_out, n), frv.write(inv[bool(flags & IM)][:n], bool(flags & OM)), (n, flags))
        assert (host(d_in) == words[:n]).all()
    d_io = filled(n)
    d_io[:n] = dev(words[:n])
    sync()
    ctx.fr_batch_inverse_device(d_io.data_ptr(), d_io.data_ptr(), n, IM | OM)  # in place
    same(host(d_io, n), frv.write(inv[True][:n], True), (n, "in place"))


# 2
def test_batch_inverse_zeros_everywhere(ctx, ref):
    pats, words, inv = ref
    n = 2 * 64 * G + 1
    zeros = [0, R, 2 * R, 5 * R]
    chain = [64 * G + 3 + 64 * s for s in range(G)]  # the chain of lane 3 of the second wave
    places = {"first of a chain": [0, chain[0], 2 * 64 * G], "last of a chain": [64 * (G - 1), chain[-1]], "a whole chain": chain,
              "a whole wave step": list(range(64, 128)), "every second element": list(range(0, n, 2)), "all": list(range(n))}
    places.update({"place %d of a chain" % s: [chain[s]] for s in range(1, G - 1)})
    want = frv.write(inv[False][:n])
    for name, at in places.items():
        mixed = list(pats[:n])
        for t, i in enumerate(at):
            mixed[i] = zeros[t % 4]
        d_in, d_out = dev(frv.to_words(mixed)), filled(n)
        sync()
        ctx.fr_batch_inverse_device(d_in.data_ptr(), d_out.data_ptr(), n)
        got = host(d_out, n)
        hit = np.zeros(n, bool)
        hit[at] = True
        assert not got[hit].any(), name                 # zero in, zero out
        assert (got[~hit] == want[~hit]).all(), name    # every neighbour still exact
    edge = [(1 << 256) - 1, R - 1, R + 1, 1, 2 * R + 7]  # inputs >= r are read modulo r
    assert ctx.fr_batch_inverse(frv.to_words(edge)).tolist() == frv.write(frv.batch_inverse(edge)).tolist()


# 3
def test_batch_inverse_host_form_equals_device_form(ctx, ref):
    pats, words, inv = ref
    for n, flags in ((1, 0), (64 * G + 1, IM), (B + 1, OM), (BIG, IM | OM)):
        same(ctx.fr_batch_inverse(words[:n], flags), frv.write(inv[bool(flags & IM)][:n], bool(flags & OM)), (n, flags))
    a = words[:300].copy()
    assert ctx.fr_batch_inverse(a, 0, out=a) is not None and (a == frv.write(inv[False][:300])).all()  # out == in


# 4
@pytest.mark.parametrize("n", sorted({1, 63, 64, 65, 1023, 1024, 1025, PB - 1, PB + 1, BIG}))
def test_powers_sizes(ctx, n):
    tau, scale = frv.patterns(0xF5ED, 2)
    for flags, first, s in ((0, 0, None), (OM, 5, scale)):
        d_out = filled(n)
        sync()
        ctx.fr_powers_device(tau, d_out.data_ptr(), n, scale=s, first=first, flags=flags)
        same(host(d_out, n), frv.write(frv.powers(tau, n, 1 if s is None else s, first), bool(flags & OM)), (n, flags))


# 5
def test_powers_bases_firsts_and_pieces(ctx):
    tau, scale = frv.patterns(0xF5EE, 2)
    n = 1024 + 65
    for base in (0, 1, R - 1, R, R + 2, tau):
        for first in (0, 1, (1 << 40) + 3):
            for s in (None, scale):
                d_out = filled(n)
                sync()
                ctx.fr_powers_device(base, d_out.data_ptr(), n, scale=s, first=first)
                same(host(d_out, n), frv.write(frv.powers(base, n, 1 if s is None else s, first)), (base, first, s is None))
    d_out = filled(3000)  # one vector made in two pieces
    sync()
    ctx.fr_powers_device(tau, d_out.data_ptr(), 1111, scale=scale)
    ctx.fr_powers_device(tau, d_out.data_ptr() + 1111 * 32, 3000 - 1111, scale=scale, first=1111)
    same(host(d_out, 3000), frv.write(frv.powers(tau, 3000, scale)), "two pieces")


# 6
@pytest.mark.parametrize("log_n", [0, 1, 2, 7, B.bit_length(), 14])
def test_lagrange(ctx, log_n):
    n, w = 1 << log_n, frv.root_of_unity(log_n)
    assert w == mh.fr_root_of_unity(log_n)
    tau = frv.patterns(0xF5EF, 1)[0]
    inside = [1, w, pow(w, n - 1, R), pow(w, n // 2 + 1, R) + R]  # (the last one spelled above r)
    cases = [(0, tau), (OM, tau), (0, inside[2])] if log_n == 14 else [(f, t) for f in (0, OM) for t in [tau, 0] + inside[:4 if f == 0 else 2]]
    for flags, t in cases:
        d_out = filled(n)
        sync()
        ctx.fr_lagrange_device(t, log_n, d_out.data_ptr(), flags)
        same(host(d_out, n), frv.write(frv.lagrange(t, log_n), bool(flags & OM)), (log_n, flags, hex(t)))


# 7
@pytest.mark.parametrize("n", [1, 65, 257, BIG])
def test_lincomb_terms_aliases_and_flags(ctx, ref, n):
    pats = ref[0]
    a, b, c = pats[:n], (pats[3:] + pats[:3])[:n], ([(1 << 256) - 1] * 3 + pats[10:] + pats[:10])[:n]  # (the largest words in c's first places)
    ka, kb, kc = frv.patterns(0xF5F0, 2) + [(1 << 256) - 1]
    wa, wb, wc = frv.to_words(a), frv.to_words(b), frv.to_words(c)
    for flags in FLAG_SETS if n < BIG else (0, IM | OM):
        m = bool(flags & IM)
        ra, rb, rc = frv.read(a, m), frv.read(b, m), frv.read(c, m)
        for present in range(4):
            for ks in ((ka, kb, kc), (None, None, None)):
                k1 = [1 if k is None else k for k in ks]
                want = frv.write(frv.lincomb(ra, k1[0], rb if present & 1 else None, k1[1], rc if present & 2 else None, k1[2]), bool(flags & OM))
                for alias in range(4) if n < BIG and ks[0] is not None else (0,):
                    if alias >= 2 and not present >> (alias - 2) & 1:
                        continue
                    d = [filled(n) for _ in range(4)]
                    for t, w in zip(d, (wa, wb, wc)):
                        t[:n] = dev(w)
                    sync()
                    out = d[alias - 1] if alias else d[3]
                    ctx.fr_lincomb_device(d[0].data_ptr(), out.data_ptr(), n, ks[0], d[1].data_ptr() if present & 1 else None, ks[1],
                                          d[2].data_ptr() if present & 2 else None, ks[2], flags)
                    same(host(out, n), want, (n, flags, present, alias))


# 8
def test_errors_leave_the_context_usable(ctx, ref):
    pats, words, inv = ref
    n = 100
    d_in, d_out = dev(words[:n]), filled(n)
    sync()
    p_in, p_out = d_in.data_ptr(), d_out.data_ptr()
    bad = [(lambda: ctx.fr_batch_inverse_device(None, p_out, n), mh.ERR_BAD_ARG), (lambda: ctx.fr_batch_inverse_device(p_in, None, n), mh.ERR_BAD_ARG),
           (lambda: ctx.fr_batch_inverse_device(p_in + 4, p_out, n), mh.ERR_BAD_ARG), (lambda: ctx.fr_batch_inverse_device(p_in, p_out + 8, n), mh.ERR_BAD_ARG),
           (lambda: ctx.fr_batch_inverse_device(p_in, p_out, n, 1), mh.ERR_BAD_ARG), (lambda: ctx.fr_batch_inverse_device(p_in, p_out, n, 8), mh.ERR_BAD_ARG),
           (lambda: ctx.fr_batch_inverse_device(p_in, p_out, 0), mh.ERR_EMPTY),
           (lambda: ctx.fr_batch_inverse(np.zeros((0, 8), np.uint32)), mh.ERR_EMPTY), (lambda: ctx.fr_batch_inverse(words[:n], 16), mh.ERR_BAD_ARG),
           (lambda: ctx.fr_powers_device(3, None, n), mh.ERR_BAD_ARG), (lambda: ctx.fr_powers_device(3, p_out + 4, n), mh.ERR_BAD_ARG),
           (lambda: ctx.fr_powers_device(3, p_out, n, flags=IM), mh.ERR_BAD_ARG), (lambda: ctx.fr_powers_device(3, p_out, 0), mh.ERR_EMPTY),
           (lambda: ctx.fr_powers_device(None, p_out, n), mh.ERR_BAD_ARG), (lambda: ctx.fr_powers_device(3, p_out, n, first=(1 << 64) - 5), mh.ERR_BAD_ARG),
           (lambda: ctx.fr_lagrange_device(3, 5, None), mh.ERR_BAD_ARG), (lambda: ctx.fr_lagrange_device(3, 5, p_out + 4), mh.ERR_BAD_ARG),
           (lambda: ctx.fr_lagrange_device(3, 29, p_out), mh.ERR_BAD_ARG), (lambda: ctx.fr_lagrange_device(3, 5, p_out, IM), mh.ERR_BAD_ARG),
           (lambda: ctx.fr_lagrange_device(None, 5, p_out), mh.ERR_BAD_ARG),
           (lambda: ctx.fr_lincomb_device(None, p_out, n), mh.ERR_BAD_ARG), (lambda: ctx.fr_lincomb_device(p_in, None, n), mh.ERR_BAD_ARG),
           (lambda: ctx.fr_lincomb_device(p_in, p_out, n, d_b=p_in + 4), mh.ERR_BAD_ARG), (lambda: ctx.fr_lincomb_device(p_in, p_out, n, d_c=p_in + 12), mh.ERR_BAD_ARG),
           (lambda: ctx.fr_lincomb_device(p_in, p_out, n, flags=1), mh.ERR_BAD_ARG), (lambda: ctx.fr_lincomb_device(p_in, p_out, 0), mh.ERR_EMPTY)]
    for i, (call, code) in enumerate(bad):
        with pytest.raises(mh.MsmError) as e:
            call()
        assert e.value.code == code, (i, str(e.value))
        assert mh.fr_vector_plan() == PLAN
    assert (host(d_out) == FILL).all()  # no failed call wrote anything
    ctx.fr_batch_inverse_device(p_in, p_out, n)
    same(host(d_out, n), frv.write(inv[False][:n]), "a correct call after the errors")
    ctx.fr_lagrange_device(7, 3, p_out)
    same(host(d_out)[:8], frv.write(frv.lagrange(7, 3)), "and another")


# 9
def test_two_streams(ctx, ref):
    import torch
    pats, words, inv = ref
    tau, scale = frv.patterns(0xF5F1, 2)
    n = BIG
    d_in, d_inv, d_pow, d_lag, d_lin = dev(words), filled(n), filled(n), filled(1 << 12), filled(n)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    sync()
    ctx.fr_batch_inverse_device(d_in.data_ptr(), d_inv.data_ptr(), n, stream=s1.cuda_stream)
    ctx.fr_powers_device(tau, d_pow.data_ptr(), n, scale=scale, stream=s2.cuda_stream)
    ctx.fr_lagrange_device(tau, 12, d_lag.data_ptr(), stream=s1.cuda_stream)
    ctx.fr_lincomb_device(d_pow.data_ptr(), d_lin.data_ptr(), n, scale, d_in.data_ptr(), tau, stream=s2.cuda_stream)  # behind the powers, on their stream
    pw = frv.powers(tau, n, scale)
    same(host(d_inv, n), frv.write(inv[False]), "stream 1: inverse")
    same(host(d_pow, n), frv.write(pw), "stream 2: powers")
    same(host(d_lag, 1 << 12), frv.write(frv.lagrange(tau, 12)), "stream 1: Lagrange")
    same(host(d_lin, n), frv.write(frv.lincomb(pw, scale, frv.read(pats), tau)), "stream 2: lincomb")


# ---- the QAP at tau: the transposed matrices times the Lagrange vector -------------------------------------------------------------------------
def load_zkey_coeffs():
    """the reference key's coefficient records (matrix, row, col, pattern) in MSM_R1CS_COEF_MONT2 form, plus a few matrix-2 records"""
    with open(os.path.join(ROOT, "tests", "golden", "zkey_r1cs_coeffs.json")) as f:
        d = json.load(f)
    coefs = [(c["matrix"], c["row"], c["col"], int.from_bytes(bytes.fromhex(c["value_le_hex"]), "little")) for c in d["coefs"]]
    m2 = lambda v: v % R * pow(1 << 512, 1, R) % R
    return coefs + [(2, 0, 1, m2(1)), (2, 1, 3, m2(R - 1)), (2, 3, 0, m2(0xC0FFEE)), (2, 3, 2, m2(5))]


def dense(coefs, rows, cols):
    """the three matrices as dictionaries (row, col) -> value, from MONT2 records"""
    un = pow(1 << 512, -1, R)
    ms = [{}, {}, {}]
    for m, r, c, v in coefs:
        assert r < rows and c < cols
        ms[m][(r, c)] = (ms[m].get((r, c), 0) + v * un) % R
    return ms


# 10
def test_adjoint_check_against_the_row_form(ctx):
    """<M^T L(tau), w> = <L(tau), M w> for each matrix: the left side is fr_lagrange_device -> transposed upload -> r1cs_eval_device, the right
    side the existing row form on a second context; no yardstick on either side"""
    coefs = load_zkey_coeffs()
    rnd = random.Random(0xAD101)
    tau, w = rnd.getrandbits(256), [rnd.getrandbits(256) for _ in range(4)]
    ctx.r1cs_upload(mh.transpose_r1cs_coefs(coefs), 4, 4, 2, mh.R1CS_COEF_MONT2)
    d_l, d_cols = filled(4), filled(12)
    sync()
    ctx.fr_lagrange_device(tau, 2, d_l.data_ptr())
    ctx.r1cs_eval_device(d_l.data_ptr(), 4, d_cols.data_ptr())
    lag, cols = frv.from_words(host(d_l, 4)), frv.from_words(host(d_cols, 12))
    with mh.MsmContext() as rows_ctx:
        rows_ctx.r1cs_upload(coefs, 4, 4, 2, mh.R1CS_COEF_MONT2)
        rows = frv.from_words(rows_ctx.r1cs_eval(frv.to_words(w), 2))
    assert sum(lag) % R == 1
    for m in range(3):
        left = sum(x * y for x, y in zip(cols[4 * m:4 * m + 4], w)) % R
        right = sum(x * y for x, y in zip(lag, rows[4 * m:4 * m + 4])) % R
        assert left == right and left != 0, m


# 11
def test_setup_scalars_to_query_points_on_one_stream(ctx):
    """Lagrange -> transposed rows -> lincomb, and powers with scale Z(tau) / delta -> the G1 fixed-base call for the A, L and H queries and the G2
    call for B2: one non-default stream, nothing crossing PCIe in between; every point against the oracle's multiple of the yardstick's scalar"""
    import torch
    coefs = load_zkey_coeffs()
    rnd = random.Random(0x5E709)
    tau, alpha, beta, gamma, delta = (rnd.randrange(1, R) for _ in range(5))
    n_vars, log_n = 4, 2
    n = 1 << log_n
    ctx.r1cs_upload(mh.transpose_r1cs_coefs(coefs), n_vars, n, log_n, mh.R1CS_COEF_MONT2)
    d_lag, d_abc, d_l, d_h = filled(n), filled(3 * n), filled(n_vars), filled(n)
    inf_bytes = lambda: torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda:0")
    pts = {q: (dev(np.full((n, 16), FILL, np.uint32)), inf_bytes()) for q in "ALH"}
    b2 = (dev(np.full((n, 32), FILL, np.uint32)), inf_bytes())
    st = torch.cuda.Stream()
    s = st.cuda_stream
    d_inv = frv.inverse(delta)
    z_over_delta = (pow(tau, n, R) - 1) * d_inv % R
    sync()
    ctx.fr_lagrange_device(tau, log_n, d_lag.data_ptr(), stream=s)
    ctx.r1cs_eval_device(d_lag.data_ptr(), n, d_abc.data_ptr(), stream=s)
    pa, pb, pc = (d_abc.data_ptr() + 32 * n * m for m in range(3))
    ctx.fr_lincomb_device(pa, d_l.data_ptr(), n_vars, beta * d_inv % R, pb, alpha * d_inv % R, pc, d_inv, stream=s)
    ctx.fr_powers_device(tau, d_h.data_ptr(), n, scale=z_over_delta, stream=s)
    g1, g2w = fb.base_words(fb.GEN), fb2.base_words(fb2.GEN)
    for q, src in (("A", pa), ("L", d_l.data_ptr()), ("H", d_h.data_ptr())):
        ctx.fixed_base_mul_device(g1, src, n, pts[q][0].data_ptr(), pts[q][1].data_ptr(), stream=s)
    ctx.fixed_base_g2_mul_device(g2w, pb, n, b2[0].data_ptr(), b2[1].data_ptr(), stream=s)
    # the yardstick's scalars
    lag = frv.lagrange(tau, log_n)
    at_tau = [[sum(v * lag[r] for (r, c), v in m.items() if c == j) % R for j in range(n_vars)] for m in dense(coefs, n, n_vars)]
    want = {"A": at_tau[0], "L": frv.lincomb(at_tau[0], beta * d_inv % R, at_tau[1], alpha * d_inv % R, at_tau[2], d_inv),
            "H": frv.powers(tau, n, z_over_delta)}
    assert any(at_tau[0]) and any(at_tau[1]) and any(at_tau[2])
    same(host(d_abc, 3 * n), frv.write(at_tau[0] + at_tau[1] + at_tau[2]), "the QAP polynomials at tau")
    torch.cuda.synchronize()
    for q in "ALH":
        xy, inf = fb.expected(want[q])
        assert (pts[q][0].cpu().numpy().view(np.uint32) == xy).all() and (pts[q][1].cpu().numpy() == inf).all(), q
    xy, inf = fb2.expected(at_tau[1])
    assert (b2[0].cpu().numpy().view(np.uint32) == xy).all() and (b2[1].cpu().numpy() == inf).all(), "B2"


# 12
def test_a_column_as_long_as_the_domain_goes_through_the_fold(ctx):
    """2^12 constraints over 2^12 variables; variable 0 (the "one" signal) is in every constraint, so its column is a row of 2^12 entries of the
    transposed matrix"""
    log_n = 12
    n = n_vars = 1 << log_n
    rnd = random.Random(0xC0105)
    coefs = []
    for i in range(n):
        coefs += [(0, i, 0, rnd.randrange(R)), (0, i, rnd.randrange(1, n_vars), 1), (1, i, rnd.randrange(n_vars), R - 1), (2, i, rnd.randrange(n_vars), rnd.randrange(R))]
    tau = rnd.randrange(R)
    info = ctx.r1cs_upload(mh.transpose_r1cs_coefs(coefs), n_vars, n, log_n)
    assert info["longest_row"] == n and info["fold_rows"] >= 1
    d_lag, d_out = filled(n), filled(3 * n)
    sync()
    ctx.fr_lagrange_device(tau, log_n, d_lag.data_ptr())
    ctx.r1cs_eval_device(d_lag.data_ptr(), n, d_out.data_ptr())
    lag = frv.lagrange(tau, log_n)
    want = [[0] * n_vars for _ in range(3)]
    for m, r, c, v in coefs:
        want[m][c] = (want[m][c] + v * lag[r]) % R
    same(host(d_out, 3 * n), frv.write(want[0] + want[1] + want[2]), "columns at tau")
