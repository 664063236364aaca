"""The yardstick of tests/test_gpu_23_g1_msm_degenerate.py checked without a GPU: every shape of tools/g1_msm_cases.py at small sizes -- the closed form
(sum s_i c_i mod r) * G against the oracle's naive MSM over the emitted words, in both forms and under a mask; the identity cases; the endomorphism
constants; the bucket-size claims of every instance the GPU test runs (exactly T entries per bucket, the count of many_pairs, the layout of coop,
the chunks of stream_meet); the Python piece rule of tools/msm_cases_common.py against the C++ of csrc/msm_planner.hpp over a sweep
(tools/piece_plan_check.cpp); and expected_lists unchanged for the G2 callers."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import g1_msm_cases as g1  # noqa: E402
import msm_cases_common as common  # noqa: E402
from oracle import bn254_oracle as orc  # noqa: E402

R, P = g1.R, g1.P
FORMS = (g1.FORM_STD, g1.FORM_MONT)
K = g1.kernel_constants()


def words_int(ws):
    return sum(int(w) << (32 * i) for i, w in enumerate(ws))


def small_shapes():
    out = [("tiled(3, 8)", g1.tiled(3, 8, 11)), ("tiled(3, 2) spread", g1.tiled(3, 2, 12, g1.spread_scalars(12))), ("tiled(1, 2)", g1.tiled(1, 2, 13)),
           ("opposite(2, 2)", g1.opposite(2, 2, 14)), ("opposite(2, 2) + 1", g1.opposite(2, 2, 15, 1)),
           ("opposite(2, 1) + 1 spread", g1.opposite(2, 1, 16, 1, g1.spread_scalars(16)[:2])), ("scalar_opposite(4)", g1.scalar_opposite(4, 17)),
           ("endo_triple(1)", g1.endo_triple(1, 18)), ("endo_triple(3)", g1.endo_triple(3, 19)), ("endo_triple(1) distinct", g1.endo_triple(1, 20, True)),
           ("endo_triple(3) distinct", g1.endo_triple(3, 21, True)), ("sign_folded(5)", g1.sign_folded(5, 22)), ("many_pairs(6)", g1.many_pairs(6, 23)),
           ("coop(6, 4)", g1.coop(6, 4, 24)), ("coop(6, 4) ragged", g1.coop(6, 4, 24, True))]
    out += [("mixed(%d)" % T, g1.mixed(T, 30 + T)) for T in (1, 2, 3, 4, 7, 8)]
    out += [("shape %s %d" % (sh, T), g1.shape_instance(sh, T)) for sh in g1.SHAPES for T in (2, 3, 8)]
    out += [("stream_meet(%d, %+d)" % (k, sg), g1.stream_meet(k, sg, 40 + k)) for k in (1, 2, 5) for sg in (1, -1)]
    for m in (2, 3, 24):
        for sign in ("same", "alt"):
            out.append((f"one_base_ramp({m}, 8, {sign})", g1.one_base_ramp(m, 8, sign)))
    out += [("mask " + lbl, g1.with_mask(inst, 60 + i)) for i, (lbl, inst) in enumerate(list(out)) if 6 <= inst.n <= 64]
    out += [("net %d: %s" % (it, combo), inst) for it in range(g1.NET_CASES) for combo, inst in [g1.net_case(it, n=(1 if it < 32 else 9) + it % 4)]]
    return out


def test_every_shape_closed_form_equals_the_oracles_naive_msm():
    shapes = small_shapes()
    assert len(shapes) > 90
    identities = 0
    for label, inst in shapes:
        exp = inst.expected()
        emitted = []
        for form in FORMS:
            b, s, inf, e = inst.emit(form)
            assert b.shape == (inst.n, 16) and s.shape == (inst.n, 8) and b.dtype == s.dtype == np.uint32 and e == exp, label
            assert inf is None or (inf.shape == (inst.n,) and inf.dtype == np.uint8), label
            assert all(words_int(row) < R for row in s), label
            out, oinf, _ = orc.msm_naive(b, s, form, inf)  # term by term over the words the GPU test will pass
            assert bool(oinf) == (exp is None) and out.tolist() == g1.expected_words(exp), (label, form)
            emitted.append(b)
        # both forms hold the same points: the Montgomery words are the standard ones times 2^256
        std, mont = emitted
        i = (7 * len(label)) % inst.n
        if std[i].any():
            x, y = words_int(std[i][:8]), words_int(std[i][8:])
            assert (y * y - x * x * x - 3) % P == 0 and (words_int(mont[i][:8]), words_int(mont[i][8:])) == (x * 2**256 % P, y * 2**256 % P), label
        identities += exp is None
    assert identities >= 8


def test_identity_cases_and_shapes_are_what_they_claim():
    assert g1.opposite(3, 5, 14).expected() is None and g1.opposite(3, 5, 14, 1).expected() is not None
    assert g1.scalar_opposite(12, 17).expected() is None and g1.endo_triple(8, 19).expected() is None and g1.endo_triple(8, 21, True).expected() is not None
    for sh in g1.SHAPES:
        for T in (2, 3, 8, 65):
            assert (g1.shape_instance(sh, T).expected() is None) == g1.shape_is_identity(sh, T)
    b, s, inf, e = g1.tiled(3, 8, 11).emit()
    assert (b[:3] == b[21:]).all() and (s[:3] == s[3:6]).all() and len({r.tobytes() for r in b}) == 3
    # -P: the same x, y negated, in either form
    b, s, inf, e = g1.opposite(4, 1, 31).emit(g1.FORM_STD)
    for j in range(4):
        assert (b[j][:8] == b[4 + j][:8]).all() and (words_int(b[j][8:]) + words_int(b[4 + j][8:])) == P
    # sign_folded: the total is twice the first half's
    inst = g1.sign_folded(5, 22)
    half = sum(s * c for s, c in zip(inst.uscal[:5], inst.ulogs[:5])) % R
    assert inst.total() == 2 * half % R and all((a + b_) % R == 0 for a, b_ in zip(inst.uscal[:5], inst.uscal[5:]))
    for sign, tot in (("same", 24 * 25 // 2), ("alt", -12)):
        assert g1.one_base_ramp(24, 8, sign).expected() == g1.product(tot * g1.RAMP_LOG)
    m = g1.with_mask(g1.opposite(3, 5, 22), 23)
    assert m.inf.any() and not m.inf.all() and 0 in m.scalars() and m.zeroed.any()


def test_endomorphism_constants_of_the_golden_file():
    lam, beta = g1.LAMBDA, g1.BETA
    assert lam != 1 and pow(lam, 3, R) == 1 and (1 + lam + lam * lam) % R == 0 and beta != 1 and pow(beta, 3, P) == 1
    logs = g1.base_logs(3, 5)
    pts = g1.point_rows(logs, g1.FORM_STD)
    phis = g1.point_rows([c * lam % R for c in logs], g1.FORM_STD)
    for a, b in zip(pts, phis):  # lambda * (x, y) = (beta x, y)
        assert words_int(b[:8]) == beta * words_int(a[:8]) % P and (a[8:] == b[8:]).all()


# ---- the claims of the instances the GPU test runs ---------------------------------------------------------------------------------------------------
def test_every_counted_instance_fills_its_buckets_alike():
    """tiled / opposite / mixed at every border: exactly T entries in every non-empty bucket, at the widths the planner gives these sizes (8 bits up
    to 2^13 points) and at 10 and 13; the largest instance holds 3300 rows"""
    borders = g1.border_sizes()
    assert borders == sorted(set(borders)) and set(g1.LONGER_SIZES) | set(g1.FORM_SIZES) | set(g1.UNFORCED_SIZES) <= set(borders) | {5, 36}
    largest = 0
    for sh in g1.SHAPES:
        for T in sorted(set(borders) | {5, 36}):
            inst = g1.shape_instance(sh, T)
            largest = max(largest, inst.n)
            assert inst.n == 3 * T
            for c in (8, 10, 13):
                per_scalar = common.unsigned_bucket_sizes(inst.uscal, None, c)  # (the three scalars once: no bucket is shared ...)
                assert set(per_scalar.values()) == {1}
            rows = np.bincount(inst.sidx, minlength=3)
            assert rows.tolist() == [T, T, T]  # ... and every scalar has T rows
    assert largest == 3300
    sizes = common.unsigned_bucket_sizes(g1.shape_instance("mixed", 7).scalars(), None, 8)
    assert set(sizes.values()) == {7}


def test_mixed_buckets_hold_what_they_claim():
    for T in (2, 7, 8, 65):
        inst = g1.shape_instance("mixed", T)
        by_scalar = {j: [inst.ulogs[p] for p, s in zip(inst.pidx.tolist(), inst.sidx.tolist()) if s == j] for j in range(3)}
        assert len(set(by_scalar[0])) == 1 and len(set(by_scalar[2])) == T
        p1 = by_scalar[1][0]
        assert by_scalar[1] == [p1 if t % 2 == 0 else R - p1 for t in range(T)] and sum(by_scalar[1]) % R == (p1 if T % 2 else 0)


def test_many_pairs_lists_more_two_entry_buckets_than_the_lane_threshold():
    inst = g1.many_pairs(4096, g1.CASE_SEED + 0x70)
    assert inst.n == 8192 and (inst.sidx[:4096] == inst.sidx[4096:]).all()
    logs = inst.logs()
    kinds = [("same" if a == b else "opposite" if (a + b) % R == 0 else "other") for a, b in zip(logs[:4096], logs[4096:])]
    assert kinds == [("same", "opposite", "other", "other")[j % 4] for j in range(4096)]  # the pairs double, cancel, or add two points
    sizes = common.unsigned_bucket_sizes(inst.scalars(), None, 16)
    two = sum(1 for v in sizes.values() if v == 2)
    # (14 full windows of ~3800 pairs that met nobody else; window 14 holds the ten bits from 224 on, 1024 buckets of ~8)
    assert two > K["MID_LANE_MIN"] and 50000 < two < 57344 and all(v % 2 == 0 for v in sizes.values())
    assert common.expected_lists(sizes.values(), 1)["mid2"] == two


@pytest.mark.parametrize("B,ragged", [(80, False), (80, True), (64, False)])
def test_coop_layout_sits_in_one_span_of_the_piece_list_writer(B, ragged):
    m = K["COOP_MIN"]
    inst = g1.coop(B, m, g1.CASE_SEED + 0x80, ragged)
    sizes = common.unsigned_bucket_sizes(inst.scalars(), None, 8)
    rows = g1.coop_rows(B, m, ragged)
    assert dict(sizes) == {(0, d): rows[d] for d in range(1, B + 1)} and max(d for _, d in sizes) < K["PLACE_COUNT_SPAN"] == 1024
    listed = sum(1 for v in sizes.values() if v >= K["COOP_MIN"])  # at piece length 1 a bucket of v entries is v pieces
    assert listed == (B if not ragged else B - B // 10) and (listed > K["COOP_MAX"]) == (B == 80) and (B != 64 or listed == K["COOP_MAX"])
    if ragged:
        assert min(sizes.values()) == m - 1
    for d in range(1, B + 1):
        pts = {int(p) for p, s in zip(inst.pidx.tolist(), inst.sidx.tolist()) if s == d - 1}
        assert len(pts) == (1 if d % 2 == 0 else rows[d])
    want = common.expected_lists(sizes.values(), 1)
    assert want == dict(long=B, mid=0, mid2=0, pieces=inst.n, partials=inst.n)


@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("k", [1, 2, 5])
def test_stream_meet_chunks_leave_and_meet_what_they_claim(k, sign):
    inst = g1.stream_meet(k, sign, g1.CASE_SEED + 0x90)
    chunk = 1 << g1.STREAM_CHUNK_LOG2
    lay = g1.stream_meet_layout(k, sign)
    assert inst.n == 3 * chunk
    logs, sc, base = inst.logs(), inst.scalars(), inst.ulogs[:3]
    held = [0, 0, 0]
    for ch in range(3):
        rows = [(sc[i], logs[i]) for i in range(ch * chunk, (ch + 1) * chunk)]
        for j in range(3):
            mine = [c for s, c in rows if s == inst.uscal[j]]
            if ch == 0:
                assert mine == [base[j]] * k
            elif ch == 1:  # the bucket opens with the affine point sign * k P_j, on a stored k P_j
                assert held[j] == k * base[j] % R and mine[0] == sign * k * base[j] % R
                assert len(mine) > K["COOP_MIN"] and all(c in (base[j], R - base[j]) for c in mine[1:])
            else:  # buckets 0 and 1: the negative of what they hold; bucket 2 holds the identity
                assert held[j] == (lay["held"] * base[j] % R if j < 2 else 0)
                assert mine[0] == ((-lay["held"] if j < 2 else -k) * base[j]) % R and mine[1:] == [base[j]] * k
            held[j] = (held[j] + sum(mine)) % R
        assert all(c == base[0] for s, c in rows if s == 0)  # the padding: zero scalars
    assert held == [k * base[0] % R, k * base[1] % R, 0]
    # no two of the three scalars share a digit at the width of these sizes
    assert set(common.unsigned_bucket_sizes(inst.uscal[:3], None, 8).values()) == {1}


def test_one_base_ramp_fills_the_lowest_window_only():
    for c in (8, 11):
        for m in (2, 3, (1 << c) - 1):
            inst = g1.one_base_ramp(m, c, "alt")
            sizes = common.unsigned_bucket_sizes(inst.scalars(), None, c)
            assert sorted(sizes) == [(0, d) for d in range(1, m + 1)] and set(sizes.values()) == {1}


# ---- the piece rule ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("c++") is None and shutil.which("hipcc") is None, reason="no C++ compiler on PATH")
def test_python_piece_rule_equals_the_planner_over_a_sweep(tmp_path):
    exe = tmp_path / "piece_plan_check"
    cxx = ["c++"] if shutil.which("c++") else ["hipcc", "-x", "c++"]
    subprocess.run(cxx + ["-O2", "-std=c++17", os.path.join(ROOT, "tools", "piece_plan_check.cpp"), "-o", str(exe)], check=True, capture_output=True, timeout=600)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, check=True)
    seen = {"P": 0, "M": 0, "S": 0}
    for line in r.stdout.splitlines():
        kind, *v = line.split()
        v = [int(x) for x in v]
        seen[kind] += 1
        if kind == "P":
            assert common.make_piece_plan(v[0], v[1], v[2], v[3]) == (v[4], v[5]), line
        elif kind == "M":
            assert common.effective_pmax(v[0], v[1], v[2]) == v[3], line
        else:
            assert common.effective_psplit(v[0], v[1], v[2]) == v[3], line
    assert seen["P"] > 10000 and seen["M"] > 70000 and seen["S"] > 1000
    assert (common.PIECE_BINS_MAX, common.SPARSE_BUCKETS_MAX, common.SPLIT_ENTRIES_SHIFT) == (K["PIECE_BINS_MAX"], K["SPARSE_BUCKETS_MAX"], K["SPLIT_ENTRIES_SHIFT"])


def test_piece_split_covers_a_bucket_exactly_on_every_branch():
    seen = set()
    for pmax in (1, 2, 8, 9, 32):
        for run in (1, 8, 16):
            for equal in (False, True):
                if run > pmax:  # (make_piece_plan never plans runs longer than a whole bucket)
                    continue
                for sz in list(range(1, 300)) + [511, 512, 513, 1024, 1100, 5000]:
                    m, q = common.piece_split(sz, pmax, run, equal)
                    br = common.piece_branch(sz, pmax, run, equal)
                    seen.add(br)
                    assert m >= 1 and (m - 1) * q < sz <= m * q and (m == 1) == (br == "whole")
                    if br == "equal":  # ceil(sz / pmax) pieces of one length (or one shorter rest), none above pmax
                        assert m == -(-sz // pmax) and q <= pmax and q == -(-sz // m)
                    elif br == "pmax":
                        assert q == pmax
                    elif br == "psplit":
                        assert q == run and sz > common.LONG_SPAN * pmax
    assert seen == {"whole", "equal", "pmax", "psplit"}
    # the LONG_SPAN x pmax border itself
    assert common.piece_branch(8 * 9, 9, 8, True) == "equal" and common.piece_branch(8 * 9 + 1, 9, 8, True) == "psplit"


def test_unforced_rule_takes_its_three_branches_at_the_sizes_the_gpu_test_runs():
    """tiled(3, T) / mixed(T) on 8-bit plain digits: a whole bucket (T = 8), equal cuts under a raised pmax (36, 130), runs of psplit (1100)"""
    got = {}
    for T in g1.UNFORCED_SIZES:
        inst = g1.shape_instance("tiled", T)
        sizes = common.unsigned_bucket_sizes(inst.uscal, None, 8)
        entries, nonempty = T * len(sizes), len(sizes)
        plan = g1.plain_plan_triple(inst.n, 8)
        assert common.make_piece_plan(*plan) == (8, 8)
        pmax, run, equal = common.device_lengths(None, plan, entries, nonempty)
        got[T] = (common.piece_branch(T, pmax, run, equal),) + common.piece_split(T, pmax, run, equal)
        lists = common.expected_lists([T] * nonempty, plan=plan)
        m = got[T][1]
        assert lists["pieces"] == m * nonempty and lists["partials"] == (m * nonempty if m > 1 else 0)
    assert got == {8: ("whole", 1, 8), 36: ("equal", 4, 9), 130: ("equal", 5, 26), 1100: ("psplit", 138, 8)}


def old_expected_lists(sizes, piece_len):
    """expected_lists as tools/g2_msm_cases.py had it before the rule was shared"""
    out = dict(long=0, mid=0, pieces=0, partials=0, mid2=0)
    for sz in sizes:
        m = 1 if sz <= piece_len else (sz + piece_len - 1) // piece_len
        out["pieces"] += m
        if m == 1:
            continue
        out["partials"] += m
        if m == 2:
            out["mid2"] += 1
        elif m < 8:
            out["mid"] += 1
        else:
            out["long"] += (m + 1023) // 1024
    return out


def test_expected_lists_is_unchanged_for_the_g2_callers():
    import g2_msm_cases as gc
    assert gc.expected_lists is common.expected_lists and gc.unsigned_bucket_sizes is common.unsigned_bucket_sizes
    assert gc.spread_scalars is common.spread_scalars and gc.seeded_scalars is common.seeded_scalars and issubclass(gc.Instance, common.Instance)
    for ell in (1, 2, 3, 7, 26, 1024):
        for sizes in ([2] * 5, [5] * 3, [8, 130, 1100], list(range(1, 70)), [1024, 1025, 2048, 2049, 8191, 8192, 8193, 20000], [ell, ell + 1, 8 * ell, 8 * ell + 1]):
            assert gc.expected_lists(sizes, ell) == old_expected_lists(sizes, ell), (ell, sizes)
