"""BN254 G2 MSM on repeated, opposite and cancelling points (-m gpu): the data flow of the G2 point side -- k_g2_accumulate, k_g2_combine (the
two-piece list, the 3..7-piece list, the 128-lane LDS tree of one segment, the fold of several segments), k_pair_level<PointG2>,
k_g2_reduce_bits and the host finish -- with operands that send xyzz2_madd / xyzz2_add through their doubling, cancelling and identity
branches at every one of those places.  tests/test_gpu_7_g2.py runs pairwise distinct bases above n = 16; tests/test_gpu_15_g2_ops.py proves the
group law op by op.  Here every base is c_i * G2 with a known logarithm, so the expected value of an instance is one product by the independent
Python law (tools/g2_msm_cases.py, checked without a GPU by tests/test_g2_msm_cases_cpu.py); every result is compared word for word.

Forced piece lengths (MSM_HIP_PIECE_LEN) are a knob of the hooks build, read when the context is made: set before th.HooksContext().

Against a scratch build whose xyzz2_add answers the identity for equal operands (instead of xyzz2_dbl), run once: 67 of the 79 tests here fail,
every case among them (all of case 1 on plain digits but T = 2 with whole buckets, all of cases 4 to 8); tests/test_gpu_7_g2.py fails in 11 of
its 47 (the golden edge_same_base_same_scalar, and sizes and skewed instances whose reduction happens to meet equal sums) and passes the rest,
its 2^20 and 2^22 instances included."""
import os
import sys

import numpy as np
import pytest

import mopro_msm_hip as mh
from mopro_msm_hip import testhooks as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bn254_g2_py as g2  # noqa: E402
import g2_msm_cases as gc  # noqa: E402

pytestmark = pytest.mark.gpu
PLAIN = mh.FLAG_NO_GLV | mh.FLAG_UNSIGNED_DIGITS
assert (gc.FLAG_NO_GLV, gc.FLAG_UNSIGNED_DIGITS, gc.FORM_STD, gc.FORM_MONT) == (mh.FLAG_NO_GLV, mh.FLAG_UNSIGNED_DIGITS, mh.FORM_STD, mh.FORM_MONT)
TS = [2, 5, 8, 130, 1100]
ELLS = [1, 2, 3]
SEED = 0xB2541800


def check(r, exp, what=None):
    assert r.is_infinity == (exp is None), what
    assert r.affine_std.tolist() == g2.affine_words_std(exp), what  # (the identity: 32 zero words)


def hooks_ctx(monkeypatch, piece_len, **kw):
    if piece_len is None:
        monkeypatch.delenv("MSM_HIP_PIECE_LEN", raising=False)
    else:
        monkeypatch.setenv("MSM_HIP_PIECE_LEN", str(piece_len))
    return th.HooksContext(**kw)


def plain_sizes(inst, n, wb=0):
    """entries per non-empty bucket of `inst` on a NO_GLV | UNSIGNED_DIGITS context, from the plan's window width"""
    pl = th.hooks_plan(n, wb, PLAIN)
    assert pl.glv == 0 and pl.signed_digits == 0 and pl.scalar_bits == 254
    return gc.unsigned_bucket_sizes(inst.scalars(), inst.inf, pl.window_bits)


def kind_of(entries, ell):
    m = 1 if entries <= ell else -(-entries // ell)
    return m, ("whole" if m == 1 else "mid2" if m == 2 else "mid" if m < 8 else "long")


def assert_lists(counts, sizes, ell, entries):
    """every non-empty bucket holds `entries` entries: the list its ceil(entries / ell) pieces go to was the only one used, and the counters
    are the ones the piece plan's rule gives for these buckets"""
    assert sizes and set(sizes.values()) == {entries}, "the instance must fill every non-empty bucket alike"
    B = len(sizes)
    m, kind = kind_of(entries, ell)
    assert counts == gc.expected_lists(sizes.values(), ell), (counts, entries, ell)
    if kind == "whole":
        assert counts["mid2"] == counts["mid"] == counts["long"] == counts["partials"] == 0
    elif kind == "mid2":
        assert counts["mid2"] == B > 0 and counts["mid"] == counts["long"] == 0
    elif kind == "mid":
        assert counts["mid"] == B > 0 and counts["mid2"] == counts["long"] == 0
    else:
        nseg = -(-m // 1024)
        assert counts["long"] == nseg * B > 0 and counts["mid"] == counts["mid2"] == 0 and counts["partials"] * nseg == m * counts["long"]
    return kind


# ---- case 1: repeats through every list of the combine kernel ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiled3():
    """tiled(3, T) for every T: raw instances (the scalars share no digit at any window width) and their emitted words, made once"""
    out = {}
    for T in TS:
        inst = gc.raw_tiled(3, T, SEED + 1, gc.spread_scalars(SEED + 1))
        out[T] = (inst, inst.emit(mh.FORM_MONT), inst.emit(mh.FORM_STD))
    return out


@pytest.mark.parametrize("ell", ELLS)
@pytest.mark.parametrize("T", TS)
def test_tiled_repeats_plain_digits_every_list(monkeypatch, tiled3, T, ell):
    """NO_GLV | UNSIGNED_DIGITS: every non-empty bucket holds exactly T copies of one point, cut into ceil(T / ell) pieces.  ell = 1: the combine adds
    EQUAL affine records (two-piece list, 3..7-piece list, every level of the LDS tree; T = 130: more pieces than tree lanes, unequal lane sums;
    T = 1100: two segments and the last workgroup's fold).  ell = 2, 3: k_g2_accumulate doubles and goes on, the combine doubles non-affine
    records.  The list counters say that the intended list ran."""
    inst, (bm, s, inf, exp), (bs, _, _, _) = tiled3[T]
    assert exp is not None and inf is None
    sizes = plain_sizes(inst, inst.n)
    with hooks_ctx(monkeypatch, ell, flags=PLAIN) as c:
        check(c.msm_g2(bm, s, mh.FORM_MONT), exp)
        counts = c.list_counts()
        kind = assert_lists(counts, sizes, ell, T)
        check(c.msm_g2(bs, s, mh.FORM_STD), exp)
    if ell == 1:  # the table of the lists at piece length 1
        if T == 2:
            assert counts["mid2"] > 0 and counts["mid"] == counts["long"] == 0
        elif T == 5:
            assert counts["mid"] > 0 and counts["mid2"] == counts["long"] == 0
        elif T == 8:
            assert counts["long"] > 0 and counts["partials"] == 8 * counts["long"]
        elif T == 130:
            assert counts["long"] > 0 and counts["partials"] == 130 * counts["long"]
        else:
            assert counts["long"] > 0 and counts["long"] % 2 == 0 and counts["partials"] == 550 * counts["long"]
    else:
        assert kind == {(2, 2): "whole", (2, 3): "whole", (5, 2): "mid", (5, 3): "mid2", (8, 2): "mid", (8, 3): "mid"}.get((T, ell), "long")


@pytest.mark.parametrize("ell", ELLS)
@pytest.mark.parametrize("T", TS)
def test_tiled_repeats_default_plan(monkeypatch, tiled3, T, ell):
    """the same instances on the default plan (GLV split, signed digits): only the answer is claimed"""
    inst, (bm, s, inf, exp), (bs, _, _, _) = tiled3[T]
    with hooks_ctx(monkeypatch, ell) as c:
        check(c.msm_g2(bm, s, mh.FORM_MONT), exp)
        check(c.msm_g2(bs, s, mh.FORM_STD), exp)


# ---- case 2: opposites ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def opposite3():
    out = {}
    for T in TS:
        for extra in (0, 1):
            inst = gc.raw_opposite(3, T, SEED + 2, extra, gc.spread_scalars(SEED + 2))
            out[T, extra] = (inst, inst.emit(mh.FORM_MONT))
    return out


@pytest.mark.parametrize("ell", ELLS)
@pytest.mark.parametrize("extra", [0, 1])
@pytest.mark.parametrize("T", TS)
def test_opposite_copies_every_list(monkeypatch, opposite3, T, extra, ell):
    """P_j T (+ 1) times and -P_j T times under the same scalar.  extra = 0: every bucket and the instance sum to the identity -- pieces that
    cancel, identity records through the two-piece list, the 3..7-piece list and the tree; extra = 1: every bucket passes through the identity and
    ends at P_j.  On plain digits a bucket holds 2 T + extra entries: the counters name the list; then the default plan."""
    inst, (bm, s, inf, exp) = opposite3[T, extra]
    assert (exp is None) == (extra == 0)
    sizes = plain_sizes(inst, inst.n)
    with hooks_ctx(monkeypatch, ell, flags=PLAIN) as c:
        check(c.msm_g2(bm, s, mh.FORM_MONT), exp)
        assert_lists(c.list_counts(), sizes, ell, 2 * T + extra)
    with hooks_ctx(monkeypatch, ell) as c:
        check(c.msm_g2(bm, s, mh.FORM_MONT), exp)


@pytest.mark.parametrize("extra", [0, 1])
def test_opposite_copies_no_forced_length(monkeypatch, extra):
    inst = gc.raw_opposite(3, 130, SEED + 3, extra)
    for form in (mh.FORM_STD, mh.FORM_MONT):
        b, s, inf, exp = inst.emit(form)
        assert (exp is None) == (extra == 0)
        for flags in (0, PLAIN):
            with hooks_ctx(monkeypatch, None, flags=flags) as c:
                check(c.msm_g2(b, s, form), exp, (form, flags))


# ---- case 3: global cancellation -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx_default():
    c = mh.MsmContext()
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_noglv():
    c = mh.MsmContext(flags=mh.FLAG_NO_GLV)
    yield c
    c.close()


def both_forms_both_contexts(inst, ctx_default, ctx_noglv, want_identity):
    for form in (mh.FORM_STD, mh.FORM_MONT):
        b, s, inf, exp = inst.emit(form)
        assert (exp is None) == want_identity
        for c in (ctx_default, ctx_noglv):
            check(c.msm_g2(b, s, form, inf), exp, (form, c.flags))


def test_scalar_opposite_total_is_the_identity(ctx_default, ctx_noglv):
    """(P_j, s_j) and (P_j, r - s_j), 64 bases: no pair meets in a bucket, the identity appears only in the reduction and the host finish"""
    both_forms_both_contexts(gc.raw_scalar_opposite(64, SEED + 4), ctx_default, ctx_noglv, True)


@pytest.mark.parametrize("distinct", [False, True])
@pytest.mark.parametrize("L", [1, 40])
def test_endomorphism_triples(ctx_default, ctx_noglv, L, distinct):
    """P, phi2(P), phi2^2(P): with one scalar for the three the sum is the identity (1 + lambda + lambda^2 = 0), and under the GLV split the
    kernel's own record phi2(P) meets the caller's base phi2(P); with three scalars an ordinary point"""
    both_forms_both_contexts(gc.raw_endo_triple(L, SEED + 5 + L, distinct), ctx_default, ctx_noglv, not distinct)


# ---- case 4: equal and opposite neighbours in the bucket reduction -----------------------------------------------------------------------------
@pytest.mark.parametrize("sign", ["same", "alt"])
@pytest.mark.parametrize("c_bits", [8, 11])
def test_one_base_ramp_equal_and_opposite_buckets(ctx_default, c_bits, sign):
    """one base P with the scalars 1 .. m on c-bit plain digits: bucket b of the lowest window holds exactly P (sign = alt: (-1)^(b+1) P), every other
    window is empty -- every pair level adds equal (opposite) neighbours, every bit sum folds equal points or identities through the shuffle tree"""
    for m in (2, 3, (1 << c_bits) - 1):
        inst = gc.raw_one_base_ramp(m, c_bits, sign)
        sizes = gc.unsigned_bucket_sizes(inst.scalars(), None, c_bits)
        assert sorted(sizes) == [(0, d) for d in range(1, m + 1)] and set(sizes.values()) == {1}
        bm, s, inf, exp = inst.emit(mh.FORM_MONT)
        bs = inst.emit(mh.FORM_STD)[0]
        assert exp is not None
        with mh.MsmContext(window_bits=c_bits, flags=PLAIN) as c:
            assert mh.plan(m, c_bits, PLAIN).window_bits == c_bits
            check(c.msm_g2(bm, s, mh.FORM_MONT), exp, m)
            check(c.msm_g2(bs, s, mh.FORM_STD), exp, m)
        check(ctx_default.msm_g2(bm, s, mh.FORM_MONT), exp, m)


# ---- case 5: masks and zero scalars among the copies -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ell", [1, None])
@pytest.mark.parametrize("shape", ["tiled(3, 8)", "opposite(3, 5)"])
def test_masked_and_zero_scalar_copies(monkeypatch, shape, ell):
    inst = gc.raw_tiled(3, 8, SEED + 6) if shape.startswith("tiled") else gc.raw_opposite(3, 5, SEED + 6)
    inst = gc.raw_with_mask(inst, SEED + 7)
    assert inst.inf.any() and 0 in inst.scalars()
    for flags in (0, PLAIN):
        with hooks_ctx(monkeypatch, ell, flags=flags) as c:
            for form in (mh.FORM_STD, mh.FORM_MONT):
                b, s, inf, exp = inst.emit(form)
                check(c.msm_g2(b, s, form, inf), exp, (form, flags))


# ---- case 6: the G2 counterpart of the reference's fixture shape at its own test size ------------------------------------------------------------
@pytest.mark.parametrize("T", [8, 128])
def test_fixture_shape_every_pair_repeated_T_times(ctx_default, ctx_noglv, T):
    """one sequence of 2^16 / T pairs (bases from g2.chain_points) repeated T times, as the reference's generator makes its G1 instances: every
    bucket that holds a point holds T copies.  Host words in both forms and device tensors, twice each, split and unsplit plan."""
    import torch
    n = 1 << 16
    inst = gc.raw_tiled(n // T, T, SEED + 8 + T)
    bm, s, inf, exp = inst.emit(mh.FORM_MONT)
    bs = inst.emit(mh.FORM_STD)[0]
    assert exp is not None and bm.shape == (n, 32) and (bm[: n // T] == bm[n - n // T:]).all() and (s[: n // T] == s[n // T: 2 * (n // T)]).all()
    db = torch.from_numpy(bm.view(np.int32)).cuda()
    ds = torch.from_numpy(s.view(np.int32)).cuda()
    torch.cuda.synchronize()
    for c in (ctx_default, ctx_noglv):
        for _ in range(2):
            check(c.msm_g2(bs, s, mh.FORM_STD), exp)
            check(c.msm_g2(bm, s, mh.FORM_MONT), exp)
            check(c.msm_g2_device(db.data_ptr(), ds.data_ptr(), n), exp)
            t = c.timings()
            assert t["num_points"] == n and t["num_adds"] > 7 * n // 8  # no duplicate was dropped


# ---- case 7: determinism on an identity result -------------------------------------------------------------------------------------------------
def test_deterministic_words_of_an_identity_result():
    b, s, inf, exp = gc.opposite(3, 5, SEED + 9)
    assert exp is None
    with mh.MsmContext(flags=mh.FLAG_DETERMINISTIC) as c:
        rs = [c.msm_g2(b, s, mh.FORM_MONT) for _ in range(4)]
    outs = [r.jacobian_mont.tolist() for r in rs]
    assert all(r.is_infinity for r in rs) and all(len(o) == 48 and o == outs[0] for o in outs)
    assert outs[0] == g2.jacobian_mont_words(None) and all(not r.affine_std.any() for r in rs)


# ---- case 8: a seeded net of 40 combinations ---------------------------------------------------------------------------------------------------
def test_seeded_net_of_degenerate_combinations(monkeypatch):
    """size x bases (distinct, odd rows equal to row 0, every third negated, all equal) x scalars (uniform, all equal, three distinct, below 2^32,
    60 % zeros, all r - 1) x infinity mask x window width x digit flags x forced piece length, against the closed form"""
    seen = set()
    for it in range(gc.NET_CASES):
        combo, inst = gc.net_case(it)
        seen.add(combo["bases"])
        b, s, inf, exp = inst.emit(mh.FORM_MONT)
        with hooks_ctx(monkeypatch, combo["piece_len"], window_bits=combo["window_bits"], flags=combo["flags"]) as c:
            r = c.msm_g2(b, s, mh.FORM_MONT, inf)
        assert r.is_infinity == (exp is None) and r.affine_std.tolist() == g2.affine_words_std(exp), combo
    assert seen == set(gc.BASE_MODES)
