"""BN254 G1 MSM on repeated, opposite and cancelling points (-m gpu): the data flow of the G1 point side that has no G2 counterpart -- which partial
sum is added where.  k_piece_count / k_place_count / k_piece_scatter (the co-operative writer and its fallback), the three source forms of
k_accumulate_pieces<INTO, CHUNK, M256>, every branch of k_combine_pieces (the two-piece list folded by eight lanes and by one lane per bucket, the
3..7-piece chain, pass A below and above WAVE_ITEM_RECORDS pieces, pass B below and above WIDE_TREE_MAX, the fold of the segment sums and the reset of
long_done), k_pair_level8 / k_pair_level_wide / k_pair_tail / k_reduce_bits_wide -- with operands that send the group law through its doubling,
cancelling and identity branches at every one of those places.  Every base is c_i * G with a known logarithm (tools/g1_msm_cases.py, checked
without a GPU by tests/test_g1_msm_cases_cpu.py), every result is compared word for word with the closed form, every counter assertion is exact
against the piece rule written in Python integers (tools/msm_cases_common.py: expected_lists).

The knobs (MSM_HIP_PIECE_LEN, MSM_HIP_MID_LANE_MIN, MSM_HIP_DEVICE_CHUNK_LOG2) belong to the hooks build and are read when the context is made: set
before th.HooksContext().  PLAIN = NO_GLV | UNSIGNED_DIGITS: the three scalars of tiled / opposite / mixed share no digit at any width, so every
non-empty bucket holds exactly T entries.  opposite at bucket size T is T // 2 copies of P and of -P and one more P for odd T; mixed puts a
repeated point, an alternating P / -P and T distinct points into the three buckets of every window.

Left out: the fold of MORE than WIDE_TREE_MAX segment sums (fold_partials' count > CAP arm on the segment sums) needs more than 2^18 pieces in one
bucket.  stream_meet's meeting is the FIRST addition into a bucket where the sort keeps the row order inside a bucket; the answer is claimed either way.

Measured on one MI355X, one session: this file 122 tests in 8.0 s of wall time, slowest case 1.9 s (the first test of the process: library load and
first context; the net 1.1 s, the streamed instances' fixture 0.9 s, every other case below 0.15 s); tests/test_gpu_18_g2_msm_degenerate.py, the yardstick, 79 tests in 5.8 s on the same
machine.  Nothing failed on the real library.

Would the tests fail?  Four scratch builds of the hooks library with ONE value-only change each (no index, loop bound or address changed), the build
standing in for both libraries, run once; failures in this file (122 tests) / in tests/test_gpu_1_parity.py + tests/test_gpu_5_reference_fixture_shape.py
(115 tests, the G1 MSM tests that existed before; one more of them fails from the swap of the libraries alone and is not counted):
  (i)   xyzz_add answers the identity for equal operands:                   102 / 32
  (ii)  the lane form of the two-piece list adds p0 + p0:                     2 / 14   (the many_pairs case and the lane form beside the chain on mixed(2))
  (iii) pass A's lanes start from the identity, not their first record:      58 / 32
  (iv)  fold_partials' count > CAP arm drops each lane's first record:       20 / 16
(ii) first failed one test only: many_pairs then repeated every ROW, and p0 + p0 is p0 + p1 for equal points.  Its second rows now repeat, negate or
replace the base; (i), (iii) and (iv) were counted before that change.
"""
import os
import sys

import numpy as np
import pytest

import mopro_msm_hip as mh
from mopro_msm_hip import testhooks as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import g1_msm_cases as g1  # noqa: E402
import msm_cases_common as common  # noqa: E402

pytestmark = pytest.mark.gpu
PLAIN = mh.FLAG_NO_GLV | mh.FLAG_UNSIGNED_DIGITS
TABLE = mh.FLAG_WINDOW_TABLE
assert (g1.FLAG_NO_GLV, g1.FLAG_UNSIGNED_DIGITS, g1.FORM_STD, g1.FORM_MONT) == (mh.FLAG_NO_GLV, mh.FLAG_UNSIGNED_DIGITS, mh.FORM_STD, mh.FORM_MONT)
K = g1.kernel_constants()
BORDERS = g1.border_sizes()
SEED = g1.CASE_SEED
KNOBS = ("MSM_HIP_PIECE_LEN", "MSM_HIP_MID_LANE_MIN", "MSM_HIP_DEVICE_CHUNK_LOG2")


def check(r, exp, what=None):
    assert r.is_infinity == (exp is None), what
    assert r.affine_std.tolist() == g1.expected_words(exp), what  # (the identity: 16 zero words)


def hooks_ctx(monkeypatch, piece_len, mid_lane_min=None, device_chunk_log2=None, **kw):
    for name, v in zip(KNOBS, (piece_len, mid_lane_min, device_chunk_log2)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))
    return th.HooksContext(**kw)


def plain_plan(n, wb=0):
    pl = th.hooks_plan(n, wb, PLAIN)
    assert pl.glv == 0 and pl.signed_digits == 0 and pl.scalar_bits == 254 and pl.table_factor == 1
    return pl


def plain_sizes(inst, wb=0):
    """entries per non-empty bucket of `inst` on a PLAIN context, from the plan's window width (the unique scalars once, times their rows)"""
    pl = plain_plan(inst.n, wb)
    rows = np.bincount(inst.sidx, minlength=len(inst.uscal)).tolist()
    if inst.inf is not None:
        return common.unsigned_bucket_sizes(inst.scalars(), inst.inf, pl.window_bits)
    sizes = {}
    for j, s in enumerate(inst.uscal):
        for key in common.unsigned_bucket_sizes([s], None, pl.window_bits):
            sizes[key] = sizes.get(key, 0) + rows[j]
    return sizes


def kind_of(entries, ell):
    m = 1 if entries <= ell else -(-entries // ell)
    return m, ("whole" if m == 1 else "mid2" if m == 2 else "mid" if m < K["LONG_SPAN"] else "long")


def assert_lists(counts, sizes, ell, entries):
    """every non-empty bucket holds `entries` entries: the list its ceil(entries / ell) pieces go to was the only one used, and the counters
    are the ones the piece rule gives for these buckets"""
    assert sizes and set(sizes.values()) == {entries}, "the instance must fill every non-empty bucket alike"
    B = len(sizes)
    m, kind = kind_of(entries, ell)
    assert counts == common.expected_lists(sizes.values(), ell), (counts, entries, ell)
    if kind == "whole":
        assert counts["mid2"] == counts["mid"] == counts["long"] == counts["partials"] == 0 and counts["pieces"] == B
    elif kind == "mid2":
        assert counts["mid2"] == B > 0 and counts["mid"] == counts["long"] == 0 and counts["partials"] == 2 * B
    elif kind == "mid":
        assert counts["mid"] == B > 0 and counts["mid2"] == counts["long"] == 0 and counts["partials"] == m * B
    else:
        nseg = -(-m // K["LONG_SEG"])
        assert counts["long"] == nseg * B > 0 and counts["mid"] == counts["mid2"] == 0 and counts["partials"] == m * B
    return kind


@pytest.fixture(scope="module")
def shapes():
    """every (shape, T) the file runs: the raw instance, its words in both forms, its bucket sizes on the PLAIN plan -- made once"""
    cache = {}

    def get(shape, T):
        if (shape, T) not in cache:
            inst = g1.shape_instance(shape, T)
            bm, s, inf, exp = inst.emit(mh.FORM_MONT)
            bs = inst.emit(mh.FORM_STD)[0]
            assert inf is None and (exp is None) == g1.shape_is_identity(shape, T)
            sizes = plain_sizes(inst)
            assert set(sizes.values()) == {T} and inst.n == 3 * T <= 3300  # before anything runs
            cache[shape, T] = (inst, bm, bs, s, exp, sizes)
        return cache[shape, T]
    return get


@pytest.fixture(scope="module")
def device_words():
    """(bases, scalars, inf) -> device tensors (Montgomery words), kept alive by the caller"""
    import torch

    def put(bm, s, inf=None):
        db = torch.from_numpy(np.ascontiguousarray(bm).view(np.int32)).cuda()
        ds = torch.from_numpy(np.ascontiguousarray(s).view(np.int32)).cuda()
        di = None if inf is None else torch.from_numpy(np.ascontiguousarray(inf, dtype=np.uint8)).cuda()
        torch.cuda.synchronize()
        return db, ds, di
    return put


# ---- a: every list of the combine kernel, forced piece length ------------------------------------------------------------------------------------
LENGTHS = [(T, 1) for T in BORDERS] + [(T, ell) for ell in g1.LONGER_PIECES for T in g1.LONGER_SIZES]


@pytest.mark.parametrize("shape", g1.SHAPES)
@pytest.mark.parametrize("T,ell", LENGTHS)
def test_every_list_forced_piece_length(monkeypatch, shapes, shape, T, ell):
    """PLAIN digits: every non-empty bucket holds exactly T entries, cut into ceil(T / ell) pieces.  ell = 1: the combine adds affine records -- equal
    (tiled), opposite (opposite), and both beside ordinary ones in one wavefront (mixed) -- through the named list only; ell = 2, 3: the accumulation
    doubles or cancels and goes on, the combine meets non-affine equal records and identities.  Twice on one context (long_done, the piece histogram
    and the bin cursors clean themselves), then the default plan (GLV split, signed digits) under the same forced length: the answer only."""
    inst, bm, bs, s, exp, sizes = shapes(shape, T)
    with hooks_ctx(monkeypatch, ell, flags=PLAIN) as c:
        for rep in range(2):
            check(c.msm(bm, s, mh.FORM_MONT), exp, rep)
            counts = c.list_counts()
            kind = assert_lists(counts, sizes, ell, T)
        check(c.msm(bs, s, mh.FORM_STD), exp)
        assert c.list_counts() == counts
    if ell == 1:  # the table of the borders, by the constants' names
        m = T
        want = ("mid2" if m == 2 else "mid" if m < K["LONG_SPAN"] else "long")
        assert kind == want
        if kind == "long":
            assert counts["long"] == len(sizes) * (2 if m > K["LONG_SEG"] else 1)
    with hooks_ctx(monkeypatch, ell) as c:
        check(c.msm(bm, s, mh.FORM_MONT), exp)
        check(c.msm(bs, s, mh.FORM_STD), exp)


# ---- b: every source form of the accumulation ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [PLAIN, 0], ids=["plain", "default"])
@pytest.mark.parametrize("shape", g1.SHAPES)
@pytest.mark.parametrize("T", g1.FORM_SIZES)
def test_every_source_form(monkeypatch, shapes, device_words, shape, T, flags):
    """the host call on arkworks words (the M256 gather) and on standard words (internal records), device pointers, a resident set, a resident set
    under FLAG_WINDOW_TABLE (plain digits carry no table: the ordinary plan again).  PLAIN: piece length 1 and the counters after every form;
    the default plan: its own lengths, the answer."""
    inst, bm, bs, s, exp, sizes = shapes(shape, T)
    ell = 1 if flags == PLAIN else None
    db, ds, _ = device_words(bm, s)

    def lists(c, what):
        if flags == PLAIN:
            assert_lists(c.list_counts(), sizes, ell, T), what

    with hooks_ctx(monkeypatch, ell, flags=flags) as c:
        check(c.msm(bm, s, mh.FORM_MONT), exp, "mont")
        lists(c, "mont")
        check(c.msm(bs, s, mh.FORM_STD), exp, "std")
        lists(c, "std")
        check(c.msm_device(db.data_ptr(), ds.data_ptr(), inst.n), exp, "device")
        lists(c, "device")
        for form, b in ((mh.FORM_MONT, bm), (mh.FORM_STD, bs)):
            c.upload_bases(b, form)
            check(c.msm_resident(s), exp, ("resident", form))
            lists(c, "resident")
    with hooks_ctx(monkeypatch, ell, flags=flags | TABLE) as c:
        c.upload_bases(bm, mh.FORM_MONT)
        for rep in range(2):
            check(c.msm_resident(s), exp, ("table", rep))
        lists(c, "table")


# ---- c: the two-piece list, one lane per bucket and eight ------------------------------------------------------------------------------------------
def test_two_piece_list_by_lanes_and_by_eight_lane_groups(monkeypatch):
    inst = g1.many_pairs(4096, SEED + 0x70)
    bm, s, inf, exp = inst.emit(mh.FORM_MONT)
    assert plain_plan(inst.n, 16).window_bits == 16
    sizes = plain_sizes(inst, 16)
    want = common.expected_lists(sizes.values(), 1)
    assert want["mid2"] == sum(1 for v in sizes.values() if v == 2) > K["MID_LANE_MIN"] == 32768
    results = []
    for lane_min in (None, want["mid2"] + 1):  # the default threshold: one lane per bucket; above the count: the eight-lane form folds the same list
        with hooks_ctx(monkeypatch, 1, mid_lane_min=lane_min, window_bits=16, flags=PLAIN) as c:
            for rep in range(2):
                r = c.msm(bm, s, mh.FORM_MONT)
                check(r, exp, (lane_min, rep))
                counts = c.list_counts()
                assert counts == want and counts["mid2"] > K["MID_LANE_MIN"]
            results.append(r.affine_std.tolist())
    assert results[0] == results[1]


@pytest.mark.parametrize("shape", ["tiled", "mixed"])
def test_two_piece_list_lane_form_on_a_handful_of_buckets(monkeypatch, shapes, shape):
    """MSM_HIP_MID_LANE_MIN = 0: the lane form whenever a two-piece bucket exists.  T = 2: only that list; then one instance whose buckets hold 2 and 5
    entries, the 3..7-piece chain beside it"""
    inst, bm, bs, s, exp, sizes = shapes(shape, 2)
    with hooks_ctx(monkeypatch, 1, mid_lane_min=0, flags=PLAIN) as c:
        for rep in range(2):
            check(c.msm(bm, s, mh.FORM_MONT), exp)
            assert assert_lists(c.list_counts(), sizes, 1, 2) == "mid2"
        check(c.msm(bs, s, mh.FORM_STD), exp)
    sc = g1.spread_scalars(SEED + 0x71)
    both = g1.Instance(g1.base_logs(2, SEED + 0x71), [0, 0, 1, 1, 1, 1, 1], sc[:2], [0, 0, 1, 1, 1, 1, 1])
    b, s2, _, e2 = both.emit(mh.FORM_MONT)
    sz = plain_sizes(both)
    assert sorted(set(sz.values())) == [2, 5]
    with hooks_ctx(monkeypatch, 1, mid_lane_min=0, flags=PLAIN) as c:
        check(c.msm(b, s2, mh.FORM_MONT), e2)
        counts = c.list_counts()
        assert counts == common.expected_lists(sz.values(), 1) and counts["mid2"] > 0 and counts["mid"] > 0 and counts["long"] == 0


# ---- d: the device-side rules over the host's plan, no forced length -------------------------------------------------------------------------------
UNFORCED_BRANCH = {8: "whole", 36: "equal", 130: "equal", 1100: "psplit"}  # a whole bucket, equal cuts under a raised pmax, runs of psplit


@pytest.mark.parametrize("shape", ["tiled", "mixed"])
@pytest.mark.parametrize("T", g1.UNFORCED_SIZES)
def test_unforced_lengths_follow_the_piece_rule(monkeypatch, shapes, shape, T):
    """effective_pmax (with PSPLIT_EQUAL equal cuts), effective_psplit and piece_split as the device applied them: the counters equal the Python rule
    for the host's plan and the entries / non-empty buckets the two-level sort counts"""
    inst, bm, bs, s, exp, sizes = shapes(shape, T)
    pl = plain_plan(inst.n)
    plan = g1.plan_triple(pl)
    assert plan == g1.plain_plan_triple(inst.n, pl.window_bits)
    pmax, run, equal = common.device_lengths(None, plan, sum(sizes.values()), len(sizes))
    assert set(UNFORCED_BRANCH) == set(g1.UNFORCED_SIZES) and common.piece_branch(T, pmax, run, equal) == UNFORCED_BRANCH[T]  # the rule takes its three branches among these T
    want = common.expected_lists(sizes.values(), plan=plan)
    with hooks_ctx(monkeypatch, None, flags=PLAIN) as c:
        for rep in range(2):
            check(c.msm(bm, s, mh.FORM_MONT), exp)
            assert c.list_counts() == want, (T, pmax, run, equal)
        check(c.msm(bs, s, mh.FORM_STD), exp)
        assert c.list_counts() == want


# ---- e: the co-operative writer of the piece list and its fallback ---------------------------------------------------------------------------------
@pytest.mark.parametrize("B,ragged", [(80, False), (80, True), (64, False)])
def test_cooperative_piece_writer_and_its_fallback(monkeypatch, B, ragged):
    """B buckets of COOP_MIN pieces in ONE workgroup of k_piece_scatter: 80 is more than the COOP_MAX it lists (the rest are written by their owner
    threads), 64 exactly COOP_MAX; ragged: every tenth bucket has one piece less and is never listed (72 are).  Even digits repeat one point"""
    inst = g1.coop(B, K["COOP_MIN"], SEED + 0x80, ragged)
    bm, s, inf, exp = inst.emit(mh.FORM_MONT)
    bs = inst.emit(mh.FORM_STD)[0]
    assert plain_plan(inst.n, 8).window_bits == 8
    sizes = plain_sizes(inst, 8)
    want = common.expected_lists(sizes.values(), 1)
    assert want == dict(long=B, mid=0, mid2=0, pieces=inst.n, partials=inst.n) and (sum(v >= K["COOP_MIN"] for v in sizes.values()) > K["COOP_MAX"]) == (B == 80)
    with hooks_ctx(monkeypatch, 1, window_bits=8, flags=PLAIN) as c:
        for rep in range(2):
            check(c.msm(bm, s, mh.FORM_MONT), exp, rep)
            assert c.list_counts() == want
        check(c.msm(bs, s, mh.FORM_STD), exp)
    with hooks_ctx(monkeypatch, 1, window_bits=8) as c:
        check(c.msm(bm, s, mh.FORM_MONT), exp)


# ---- f: accumulation INTO the buckets: streamed host chunks, point ranges of a device-resident instance --------------------------------------------
def stream_instances():
    out = [("stream_meet(%d, %+d)" % (k, sg), g1.stream_meet(k, sg, SEED + 0x90)) for k in (1, 2, 5) for sg in (1, -1)]
    sc = g1.spread_scalars(SEED + 0x91)
    return out + [("tiled(3, 200)", g1.tiled(3, 200, SEED + 0x91, sc)), ("opposite(3, 100, 1)", g1.opposite(3, 100, SEED + 0x91, 1, sc))]


@pytest.fixture(scope="module")
def streams():
    return [(label, inst, inst.emit(mh.FORM_MONT), inst.emit(mh.FORM_STD)[0]) for label, inst in stream_instances()]


@pytest.mark.parametrize("flags", [PLAIN, 0], ids=["plain", "default"])
@pytest.mark.parametrize("ell", [1, None])
def test_streamed_chunks_meet_the_stored_bucket(monkeypatch, streams, ell, flags):
    """stream_chunk_log2 = 8: chunk 1 leaves k P_j, chunk 2 opens the bucket with +k P_j (the first INTO addition doubles a stored value) or -k P_j (it
    cancels), chunk 3 meets the negative of a long-accumulated value and an identity bucket.  Piece length 1: chunk 2's buckets go through the
    co-operative writer with PF_FIRST on their first piece"""
    with hooks_ctx(monkeypatch, ell, flags=flags, stream_chunk_log2=g1.STREAM_CHUNK_LOG2) as c:
        for label, inst, (bm, s, inf, exp), bs in streams:
            for form, b in ((mh.FORM_MONT, bm), (mh.FORM_STD, bs)):
                check(c.msm(b, s, form), exp, (label, form))
                assert c.timings()["stream_chunks"] == -(-inst.n // 256) == 3, label


@pytest.mark.parametrize("flags", [PLAIN, mh.FLAG_NO_GLV], ids=["plain", "noglv"])
@pytest.mark.parametrize("ell", [1, None])
def test_device_point_ranges_meet_the_stored_bucket(monkeypatch, streams, device_words, ell, flags):
    """MSM_HIP_DEVICE_CHUNK_LOG2 = 8 on an unsplit plan: msm_device cuts the instance into point ranges that accumulate INTO the bucket array"""
    with hooks_ctx(monkeypatch, ell, device_chunk_log2=8, flags=flags) as c:
        for label, inst, (bm, s, inf, exp), bs in streams:
            db, ds, _ = device_words(bm, s)
            for rep in range(2):
                check(c.msm_device(db.data_ptr(), ds.data_ptr(), inst.n), exp, (label, rep))
                assert c.timings()["stream_chunks"] == -(-inst.n // 256) == 3, label


# ---- g: the bucket reduction ---------------------------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("sign", ["same", "alt"])
@pytest.mark.parametrize("c_bits", [8, 11])
def test_one_base_ramp_equal_and_opposite_buckets(ctx_default, c_bits, sign):
    """one base P with the scalars 1 .. m on c-bit plain digits: bucket b of the lowest window holds exactly P (alt: (-1)^(b+1) P), every other window is
    empty -- equal or opposite neighbours at every level of k_pair_level8 / k_pair_level_wide / k_pair_tail, equal points and identities in every LDS
    tree of k_reduce_bits_wide"""
    for m in (2, 3, (1 << c_bits) - 1):
        inst = g1.one_base_ramp(m, c_bits, sign)
        sizes = common.unsigned_bucket_sizes(inst.scalars(), None, c_bits)
        assert sorted(sizes) == [(0, d) for d in range(1, m + 1)] and set(sizes.values()) == {1}
        bm, s, inf, exp = inst.emit(mh.FORM_MONT)
        bs = inst.emit(mh.FORM_STD)[0]
        assert exp is not None
        with mh.MsmContext(window_bits=c_bits, flags=PLAIN) as c:
            assert mh.plan(m, c_bits, PLAIN).window_bits == c_bits
            check(c.msm(bm, s, mh.FORM_MONT), exp, m)
            check(c.msm(bs, s, mh.FORM_STD), exp, m)
        check(ctx_default.msm(bm, s, mh.FORM_MONT), exp, m)


def both_forms_both_contexts(inst, ctx_default, ctx_noglv, want_identity):
    for form in (mh.FORM_STD, mh.FORM_MONT):
        b, s, inf, exp = inst.emit(form)
        assert (exp is None) == want_identity
        for c in (ctx_default, ctx_noglv):
            check(c.msm(b, s, form, inf), exp, (form, c.flags))


def test_scalar_opposite_total_is_the_identity(ctx_default, ctx_noglv):
    """(P_j, s_j) and (P_j, r - s_j), 64 bases: the identity appears only in the reduction and the host finish (unsplit), or where the halves meet (split)"""
    both_forms_both_contexts(g1.scalar_opposite(64, SEED + 0xA0), ctx_default, ctx_noglv, True)


@pytest.mark.parametrize("distinct", [False, True])
@pytest.mark.parametrize("L", [1, 40])
def test_endomorphism_triples(ctx_default, ctx_noglv, L, distinct):
    """P, phi(P), phi^2(P): with one scalar for the three the sum is the identity, and under the GLV split the kernel's own record phi(P) meets the
    caller's base phi(P); with three scalars an ordinary point"""
    both_forms_both_contexts(g1.endo_triple(L, SEED + 0xA1 + L, distinct), ctx_default, ctx_noglv, not distinct)


def test_sign_folded_rows_double_through_the_negated_digit(ctx_default, ctx_noglv):
    """(P_j, s_j) and (-P_j, r - s_j): 2 s_j P_j.  The answer only"""
    both_forms_both_contexts(g1.sign_folded(64, SEED + 0xA2), ctx_default, ctx_noglv, False)


# ---- h: masks, determinism, the net ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ell", [1, None])
@pytest.mark.parametrize("shape", ["tiled(3, 8)", "opposite(3, 5)"])
def test_masked_and_zero_scalar_copies(monkeypatch, shape, ell):
    inst = g1.tiled(3, 8, SEED + 0xB0) if shape.startswith("tiled") else g1.opposite(3, 5, SEED + 0xB0)
    inst = g1.with_mask(inst, SEED + 0xB1)
    assert inst.inf.any() and 0 in inst.scalars()
    for flags in (0, PLAIN):
        with hooks_ctx(monkeypatch, ell, flags=flags) as c:
            for form in (mh.FORM_STD, mh.FORM_MONT):
                b, s, inf, exp = inst.emit(form)
                check(c.msm(b, s, form, inf), exp, (form, flags))


def test_deterministic_words_of_an_identity_result():
    b, s, inf, exp = g1.opposite(3, 5, SEED + 0xB2).emit(mh.FORM_MONT)
    assert exp is None
    with mh.MsmContext(flags=mh.FLAG_DETERMINISTIC) as c:
        rs = [c.msm(b, s, mh.FORM_MONT) for _ in range(4)]
    outs = [r.jacobian_mont.tolist() for r in rs]
    assert all(r.is_infinity for r in rs) and all(len(o) == 24 and o == outs[0] for o in outs)
    assert all(not r.affine_std.any() for r in rs) and not any(outs[0][16:])  # (Z = 0)


def test_seeded_net_of_degenerate_combinations(monkeypatch, device_words):
    """size x bases (distinct, odd rows equal to row 0, every third negated, all equal) x scalars (uniform, all equal, three distinct, below 2^32,
    60 % zeros, all r - 1) x infinity mask x window width x digit flags x forced piece length x source form, against the closed form"""
    seen = set()
    for it in range(g1.NET_CASES):
        combo, inst = g1.net_case(it)
        seen.add((combo["bases"], combo["source"]))
        src = combo["source"]
        bm, s, inf, exp = inst.emit(mh.FORM_MONT)
        flags = combo["flags"] | (TABLE if src == "resident table" else 0)
        with hooks_ctx(monkeypatch, combo["piece_len"], window_bits=combo["window_bits"], flags=flags) as c:
            if src == "host mont":
                r = c.msm(bm, s, mh.FORM_MONT, inf)
            elif src == "host std":
                r = c.msm(inst.emit(mh.FORM_STD)[0], s, mh.FORM_STD, inf)
            elif src == "device":
                db, ds, di = device_words(bm, s, inf)
                r = c.msm_device(db.data_ptr(), ds.data_ptr(), inst.n, None if di is None else di.data_ptr())
            else:
                c.upload_bases(bm, mh.FORM_MONT, inf)
                r = c.msm_resident(s)
        assert r.is_infinity == (exp is None) and r.affine_std.tolist() == g1.expected_words(exp), combo
    assert {b for b, _ in seen} == set(g1.BASE_MODES) and {f for _, f in seen} == set(g1.SOURCE_FORMS)
