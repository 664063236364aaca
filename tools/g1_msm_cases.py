"""Inputs and expected values of the G1 MSM's tests on repeated, opposite and cancelling points (tests/test_g1_msm_cases_cpu.py,
tests/test_gpu_23_g1_msm_degenerate.py): the G1 counterpart of tools/g2_msm_cases.py.  Every base is c_i * G with a known logarithm c_i, so the
expected result of an instance is ONE product, (sum_{i not masked} s_i c_i mod r) * G, or None for the identity.  Points and products come from
the CPU oracle (oracle/bn254_oracle.py: gen_bases_from_logs, g1_scalar_mul); nothing here touches the code under test.  A point IS its
logarithm here: -P is r - c, phi(P) = (beta x, y) is lambda c (lambda, beta: tests/golden/glv_constants.json).

Every builder returns an Instance; emit(form) gives (bases n x 16 words in the requested form, scalars n x 8 words, inf mask or None, expected
affine standard-form words as a tuple of 16 or None).  Shapes as for G2 -- tiled, opposite, scalar_opposite, endo_triple, one_base_ramp,
with_mask, the seeded net -- and the ones that pin G1-only data flow: mixed, sign_folded, many_pairs, coop, stream_meet.  The index logic, the
scalars, the bucket sizes and the piece rule (expected_lists) are shared with the G2 module: tools/msm_cases_common.py."""
import json
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p_ in (HERE, ROOT):
    if p_ not in sys.path:
        sys.path.insert(0, p_)
import msm_cases_common as common  # noqa: E402
from msm_cases_common import (FLAG_NO_GLV, FLAG_UNSIGNED_DIGITS, FORM_MONT, FORM_STD, LONG_SEG, LONG_SPAN, SPREAD_BITS, R, expected_lists,  # noqa: E402,F401
                              scalar_words, seeded_scalars, spread_scalars, unsigned_bucket_sizes)
from oracle import bn254_oracle as orc  # noqa: E402

P = orc.P
assert R == orc.R_ORDER
with open(os.path.join(ROOT, "tests", "golden", "glv_constants.json")) as f_:
    _GLV = json.load(f_)
LAMBDA, BETA = int(_GLV["lambda"], 16), int(_GLV["beta"], 16)  # phi(x, y) = (BETA x, y) = LAMBDA * (x, y) on G1
_WORDS = {FORM_STD: {}, FORM_MONT: {}}  # logarithm -> the 16 words of the point, per form


def point_rows(logs, form):
    """the points logs[i] * G as n x 16 words (oracle), each logarithm multiplied once per process"""
    cache = _WORDS[form]
    new = sorted({c for c in logs if c not in cache})
    if new:
        for c, row in zip(new, orc.gen_bases_from_logs(scalar_words(new), form)):
            cache[c] = row
    return np.array([cache[c] for c in logs], np.uint32).reshape(len(logs), 16)


def product(total):
    """total * G as 16 affine standard-form words (a tuple), None for the identity"""
    total %= R
    if total == 0:
        return None
    g = np.zeros(16, np.uint32)
    g[0], g[8] = 1, 2
    words, inf = orc.g1_to_affine_std(orc.g1_scalar_mul(g, orc.int_to_words(total)))
    assert not inf
    return tuple(int(w) for w in words)


def expected_words(exp):
    return [0] * 16 if exp is None else list(exp)


class Instance(common.Instance):
    """common.Instance over G1: upts are the logarithms themselves"""

    def __init__(self, ulogs, pidx, uscal, sidx, inf=None, zeroed=None):
        ulogs = [c % R for c in ulogs]
        assert all(ulogs), "a base at infinity has no words: mask the row instead"
        super().__init__(ulogs, ulogs, pidx, uscal, sidx, inf, zeroed)

    def point_words(self, form):
        return point_rows(self.ulogs, form)

    def product(self, total):
        return product(total)


def base_logs(L, seed):
    """L logarithms, no two equal or opposite"""
    rnd, logs, seen = random.Random(seed), [], set()
    while len(logs) < L:
        c = rnd.randrange(1, R)
        if c not in seen:
            logs.append(c)
            seen.update((c, R - c))
    return logs


# ---- the shapes of the G2 module ------------------------------------------------------------------------------------------------------------------
def tiled(L, T, seed, scalars=None):
    """L distinct pairs (c_j * G, s_j) repeated T times: pair j at rows t * L + j.  Every bucket that holds a point holds T copies of it."""
    sc = list(scalars) if scalars is not None else seeded_scalars(seed, L)
    assert len(sc) == L
    idx = np.tile(np.arange(L), T)
    return Instance(base_logs(L, seed), idx, sc, idx)


def opposite(L, T, seed, extra=0, scalars=None):
    """(P_j, s_j) T + extra times and (-P_j, s_j) T times.  extra = 0: every bucket sums to the identity, and so does the instance; extra = 1: every
    bucket passes through the identity and ends at P_j.  Rows: T blocks of [P_0 .. P_{L-1}, -P_0 .. -P_{L-1}], then the extra blocks of P."""
    logs = base_logs(L, seed)
    sc = list(scalars) if scalars is not None else seeded_scalars(seed, L)
    assert len(sc) == L
    pidx = np.concatenate([np.tile(np.arange(2 * L), T), np.tile(np.arange(L), extra)]).astype(np.int64)
    return Instance(logs + [R - c for c in logs], pidx, sc, pidx % L)


def scalar_opposite(L, seed):
    """(P_j, s_j) and (P_j, r - s_j): nothing cancels inside a bucket (the digits differ), the total is the identity"""
    sc = seeded_scalars(seed, L)
    idx = np.arange(L)
    return Instance(base_logs(L, seed), np.concatenate([idx, idx]), sc + [R - s for s in sc], np.concatenate([idx, L + idx]))


def endo_triple(L, seed, distinct=False):
    """bases P_j, phi(P_j), phi^2(P_j) (logarithms c, lambda c, lambda^2 c).  distinct = False: the three carry the same scalar s_j and sum to the
    identity (1 + lambda + lambda^2 = 0 mod r); True: three scalars of their own, an ordinary point.  Under the GLV split the record phi(P_j)
    the kernel makes for the base P_j and the caller's own base phi(P_j) are the same point in two records."""
    logs = base_logs(L, seed)
    ulogs = logs + [c * LAMBDA % R for c in logs] + [c * LAMBDA * LAMBDA % R for c in logs]
    sc = seeded_scalars(seed, 3 * L if distinct else L)
    pidx = np.arange(3 * L)
    return Instance(ulogs, pidx, sc, pidx if distinct else pidx % L)


RAMP_LOG = 0x2F0C5A7E11D3B9A86C4E20197F5D3B1A0C9E8D7F6A5B4C3D2E1F0A9B8C7D6E5  # the logarithm of one_base_ramp's base


def one_base_ramp(m, c, sign="same", log=RAMP_LOG):
    """the ONE base P = log * G, m times, with the scalars 1, 2, ..., m < 2^c.  With c-bit plain digits and no GLV split, bucket b of the lowest
    window holds exactly P and every other window is empty: every pair level and every bit sum adds equal points.  sign = "alt": the base
    of row j is (-1)^j P, adjacent buckets are opposite.  Expected: (sum +-(j + 1)) * log * G."""
    assert 0 < m < (1 << c) and sign in ("same", "alt")
    pidx = np.arange(m) % 2 if sign == "alt" else np.zeros(m, np.int64)
    return Instance([log, R - log], pidx, list(range(1, m + 1)), np.arange(m))


def with_mask(inst, seed):
    """`inst` with about a quarter of its rows masked as infinity (every other one with zeroed base words) and about a sixth carrying the scalar 0"""
    inf, zeroed, uscal, sidx = common.mask_rows(inst, seed)
    return Instance(inst.ulogs, inst.pidx, uscal, sidx, inf, zeroed)


# ---- the shapes that pin G1-only data flow --------------------------------------------------------------------------------------------------------
def mixed(T, seed, scalars=None):
    """three buckets per window under one piece length, T entries each: scalar 0 carries T copies of ONE point; scalar 1 T // 2 copies of P and of -P,
    alternating, and one more P when T is odd (extra = T mod 2: the bucket sums to the identity, or passes through it and ends at P); scalar 2 T
    pairwise distinct points.  Rows: T rounds of [bucket 0's, bucket 1's, bucket 2's next entry].  With spread_scalars ordinary pairs (bucket 2),
    equal pairs (bucket 0) and opposite pairs (bucket 1) share the eight-lane groups of a wavefront in the combine kernel."""
    sc = list(scalars) if scalars is not None else spread_scalars(seed)
    assert len(sc) == 3 and T >= 1
    logs = base_logs(T + 2, seed)  # [0]: the repeated point, [1]: P (and -P at index T + 2), [2 ..]: the T distinct ones
    ulogs = logs + [R - logs[1]]
    pidx, sidx = [], []
    for t in range(T):
        pidx += [0, 1 if t % 2 == 0 else T + 2, 2 + t]  # (odd T: the last entry, at an even t, is the P that stays)
        sidx += [0, 1, 2]
    return Instance(ulogs, pidx, sc, sidx)


def sign_folded(L, seed):
    """rows (P_j, s_j) and (-P_j, r - s_j): the total is 2 sum s_j P_j.  Where the signed recoding gives r - s the digits -d of s (the default plan
    does for the halves of a split scalar), the two rows meet in one bucket as +P under +d and -P under -d: a doubling through the negated-digit path."""
    logs, sc = base_logs(L, seed), seeded_scalars(seed, L)
    idx = np.arange(L)
    return Instance(logs + [R - c for c in logs], np.concatenate([idx, L + idx]), sc + [R - s for s in sc], np.concatenate([idx, L + idx]))


def many_pairs(L, seed):
    """L random scalars below 2^SPREAD_BITS, every scalar on two rows (j and L + j): with plain 16-bit digits nearly every non-empty bucket holds
    exactly two entries.  The second row's base is the first one's again (j = 0 mod 4: the fold doubles), its negative (1 mod 4: it cancels) or another
    point (2, 3 mod 4: an ordinary addition, which a fold that read one operand twice would get wrong).  At L = 4096 more than 5 * 10^4 such buckets
    (14 full windows): more than MID_LANE_MIN."""
    rnd = random.Random(seed ^ 0x9A125)
    sc = [rnd.getrandbits(SPREAD_BITS) | 1 for _ in range(L)]
    logs = base_logs(2 * L, seed)
    ulogs = logs[:L] + [logs[j] if j % 4 == 0 else R - logs[j] if j % 4 == 1 else logs[L + j] for j in range(L)]
    idx = np.arange(L)
    return Instance(ulogs, np.concatenate([idx, L + idx]), sc, np.concatenate([idx, idx]))


def coop_rows(B, m, ragged=False):
    """rows per digit 1 .. B of coop(): m, or m - 1 for every tenth digit of the ragged variant"""
    return {d: m - 1 if ragged and d % 10 == 0 else m for d in range(1, B + 1)}


def coop(B, m, seed, ragged=False):
    """the scalars 1 .. B (one 8-bit plain digit, window 0), m rows each: even digits repeat one point, odd digits hold m distinct ones.  Rows: m rounds
    over the digits.  All B buckets lie in the first 1024-bucket span of the bucket array: ONE workgroup of the piece-list writer sees them all.
    ragged: every tenth digit has m - 1 rows."""
    assert 0 < B < 256
    rows = coop_rows(B, m, ragged)
    first, nlogs = {}, 0
    for d in range(1, B + 1):
        first[d] = nlogs
        nlogs += 1 if d % 2 == 0 else rows[d]
    logs = base_logs(nlogs, seed)
    pidx, sidx = [], []
    for t in range(m):
        for d in range(1, B + 1):
            if t < rows[d]:
                pidx.append(first[d] + (0 if d % 2 == 0 else t))
                sidx.append(d - 1)
    return Instance(logs, pidx, list(range(1, B + 1)), sidx)


STREAM_CHUNK_LOG2 = 8
STREAM_FOLLOW = 84  # copies of P_j behind the meeting row of chunk 2 (buckets 0 and 1): 85 entries, more than the co-operative writer's minimum


def stream_meet(k, sign, seed, scalars=None):
    """three chunks of 2^8 rows for a streamed call (or three point ranges of a device-resident one); bases P_0, P_1, P_2 under three scalars
    that share no digit (spread_scalars).
      chunk 1: k copies of every (P_j, s_j), padded with zero-scalar rows: bucket j is left at exactly k P_j.
      chunk 2: opens bucket j with the AFFINE point sign * k P_j -- sign = +1: the first addition INTO the bucket doubles the stored (non-affine for
               k > 1) value; -1: it cancels to the identity -- then STREAM_FOLLOW copies of P_j follow in buckets 0 and 1; in bucket 2, x copies
               of P_2 and y of -P_2 that bring it to the identity exactly.
      chunk 3: buckets 0 and 1 open with the affine negative of what they hold (the -1 meeting on a long-accumulated value), then k copies of
               P_j; bucket 2, which holds the identity, opens with -k P_2 and then takes k copies of P_2: it ends at the identity again.
    stream_meet_layout() says the same in numbers for the CPU test."""
    assert sign in (1, -1) and 1 <= k <= 40
    sc = list(scalars) if scalars is not None else spread_scalars(seed)
    logs = base_logs(3, seed)
    chunk = 1 << STREAM_CHUNK_LOG2
    lay = stream_meet_layout(k, sign)
    ulogs, pidx, sidx = list(logs), [], []

    def point(c):
        c %= R
        if c not in ulogs:
            ulogs.append(c)
        return ulogs.index(c)

    def pad():
        while len(pidx) % chunk:
            pidx.append(0)
            sidx.append(3)  # the zero scalar

    for _ in range(k):
        for j in range(3):
            pidx.append(j), sidx.append(j)
    pad()
    for j in range(3):
        pidx.append(point(sign * k * logs[j])), sidx.append(j)
    for t in range(STREAM_FOLLOW):
        for j in range(2):
            pidx.append(j), sidx.append(j)
        if t < lay["x"]:
            pidx.append(2), sidx.append(2)
        elif t < lay["x"] + lay["y"]:
            pidx.append(point(R - logs[2])), sidx.append(2)
    pad()
    for j in range(2):
        pidx.append(point(-lay["held"] * logs[j])), sidx.append(j)
    pidx.append(point(-k * logs[2])), sidx.append(2)
    for _ in range(k):
        for j in range(3):
            pidx.append(j), sidx.append(j)
    pad()
    assert len(pidx) == 3 * chunk
    return Instance(ulogs, pidx, sc + [0], sidx)


def stream_meet_layout(k, sign):
    """x, y: copies of P_2 and -P_2 in chunk 2; held: the multiple of P_j buckets 0 and 1 hold after chunk 2; final: after chunk 3 (bucket 2: 0)"""
    x = 40 - k if sign > 0 else 40
    y = 40 + k if sign > 0 else 40
    assert k + sign * k + x - y == 0 and x + y <= STREAM_FOLLOW
    held = k + sign * k + STREAM_FOLLOW
    return dict(x=x, y=y, held=held, final=k)


# ---- the seeded net: 40 combinations of size, bases, scalars, mask, window width, digit flags, forced piece length and source form ------------------
NET_SEED, NET_CASES, NET_POOL = 20261020, 40, 3200
BASE_MODES = ("distinct", "odd rows = row 0", "every third negated", "all equal")
SCALAR_MODES = ("uniform", "all equal", "three distinct", "below 2^32", "60 % zeros", "all r - 1")
SOURCE_FORMS = ("host mont", "host std", "device", "resident", "resident table")
_POOL = []


def net_pool():
    if not _POOL:
        _POOL.append(base_logs(NET_POOL, NET_SEED))
    return _POOL[0]


def net_case(it, n=None):
    """(combination, Instance) number `it` of the net; n overrides the drawn size (the CPU test checks every mode at a small one).  The
    combination is a dict of everything that was drawn: a failing case reports it whole."""
    rng = np.random.default_rng([NET_SEED, it])
    drawn = int(rng.choice([rng.integers(1, 41), rng.integers(40, 801), rng.integers(800, 3001)]))
    n = drawn if n is None else n
    off = int(rng.integers(0, NET_POOL - n + 1))
    bmode, smode = it % len(BASE_MODES), int(rng.integers(0, len(SCALAR_MODES)))
    logs = net_pool()[off:off + n]
    if bmode == 1:
        logs = [logs[0] if i % 2 else c for i, c in enumerate(logs)]
    elif bmode == 2:
        logs = [R - c if i % 3 == 2 else c for i, c in enumerate(logs)]
    elif bmode == 3:
        logs = [logs[0]] * n
    rnd = random.Random(int(rng.integers(0, 1 << 62)))
    sc = [rnd.randrange(R) for _ in range(n)]
    if smode == 1:
        sc = [sc[0]] * n
    elif smode == 2:
        sc = [sc[i % 3] for i in range(n)]
    elif smode == 3:
        sc = [s & 0xFFFFFFFF for s in sc]
    elif smode == 4:
        sc = [0 if rnd.random() < 0.6 else s for s in sc]
    elif smode == 5:
        sc = [R - 1] * n
    density = [None, 0.001, 0.05, 0.9][int(rng.integers(0, 4))]
    inf = None if density is None else (rng.random(n) < density).astype(np.uint8)
    combo = dict(case=it, n=n, offset=off, bases=BASE_MODES[bmode], scalars=SCALAR_MODES[smode], inf_density=density,
                 window_bits=int(rng.choice([0, 5, 8, 11, 13])), flags=int(rng.choice([0, FLAG_NO_GLV, FLAG_UNSIGNED_DIGITS, FLAG_NO_GLV | FLAG_UNSIGNED_DIGITS])),
                 piece_len=[None, "1", "2", "7"][int(rng.integers(0, 4))], source=SOURCE_FORMS[(it // len(BASE_MODES)) % len(SOURCE_FORMS)])
    uniq = sorted(set(logs))
    pos = {c: i for i, c in enumerate(uniq)}
    idx = np.arange(n)
    return combo, Instance(uniq, [pos[c] for c in logs], sc, idx, inf)


# ---- the kernels' constants and the instances the GPU test runs (the CPU test holds their claims) ----------------------------------------------------
def kernel_constants():
    """the borders of k_combine_pieces and k_piece_scatter, read from the headers that define them"""
    import re
    csrc = os.path.join(ROOT, "gpu-acceleration_amd", "csrc")
    with open(os.path.join(csrc, "msm_kernels.hpp")) as f:
        hdr = f.read()
    with open(os.path.join(csrc, "msm_planner.hpp")) as f:
        hdr += f.read()
    out = {}
    for name in ("LONG_SPAN", "LONG_SEG", "WAVE_ITEM_MAX", "WAVE_ITEM_RECORDS", "MID_LANE_MIN", "COOP_MIN", "COOP_MAX", "WIDE_TREE_MAX",
                 "PLACE_COUNT_SPAN", "SPARSE_BUCKETS_MAX", "PIECE_BINS_MAX", "SPLIT_ENTRIES_SHIFT"):
        m = re.search(r"constexpr (?:uint32_t|size_t)[^;]*\b%s = (\d+)" % name, hdr)
        assert m, name
        out[name] = int(m.group(1))
    return out


def border_sizes():
    """bucket sizes T whose ceil(T / 1) pieces sit on every border of the combine kernel at piece length 1, by the constants' names"""
    k = kernel_constants()
    assert (k["LONG_SPAN"], k["LONG_SEG"]) == (LONG_SPAN, LONG_SEG) and k["COOP_MIN"] == k["WAVE_ITEM_RECORDS"]
    assert k["LONG_SEG"] < 1100 <= k["LONG_SEG"] + k["WIDE_TREE_MAX"] and 2 * k["WAVE_ITEM_RECORDS"] < 130 < k["WAVE_ITEM_MAX"]
    return [2,                                   # the two-piece list
            3, k["LONG_SPAN"] - 1,               # both ends of the chain through the group's LDS record
            k["LONG_SPAN"],                      # the shortest long bucket: pass A, fewer pieces than the wavefront's records
            k["WAVE_ITEM_RECORDS"],              # pass A with every record filled by one piece; the co-operative writer's minimum
            k["WAVE_ITEM_RECORDS"] + 1,          # pass A: one lane folds two pieces before the eight-lane tree
            130,                                 # pass A: every lane folds, two lanes one piece more
            k["WAVE_ITEM_MAX"],                  # the longest bucket of pass A
            k["WAVE_ITEM_MAX"] + 1,              # pass B: one segment, more pieces than the LDS tree holds records
            k["LONG_SEG"],                       # pass B: one full segment
            k["LONG_SEG"] + 1,                   # pass B: a second segment of ONE piece, and the fold of the segment sums
            1100]                                # pass B: a second segment below WIDE_TREE_MAX pieces (staged whole), the segment fold


LONGER_PIECES = (2, 3)        # forced piece lengths beyond 1 ...
LONGER_SIZES = (5, 8, 130, 1100)  # ... at these bucket sizes
FORM_SIZES = (2, 5, 130, 1100)    # bucket sizes every source form runs
UNFORCED_SIZES = (8, 36, 130, 1100)
SHAPES = ("tiled", "opposite", "mixed")
CASE_SEED = 0xB2542300


def shape_instance(shape, T):
    """the instance of `shape` whose non-empty buckets hold exactly T entries each under plain digits of any width (three scalars that share no digit)"""
    seed = CASE_SEED + 16 * SHAPES.index(shape) + 1
    sc = spread_scalars(seed)
    if shape == "tiled":
        return tiled(3, T, seed, sc)
    if shape == "opposite":  # T // 2 copies of P_j and of -P_j, one more P_j when T is odd
        return opposite(3, T // 2, seed, T % 2, sc)
    return mixed(T, seed, sc)


def shape_is_identity(shape, T):
    return shape == "opposite" and T % 2 == 0


def plain_plan_triple(n, c):
    """(pairs, mean occupancy, total buckets) of an unsplit plan with c-bit plain digits over n points, as pipe_prepare hands them to make_piece_plan"""
    W, nb = (254 + c - 1) // c, 1 << c
    return W * n, n // nb, W * nb


def plan_triple(pl):
    """the same from an msm_plan_t without a window table"""
    return pl.num_windows * int(pl.virtual_points), int(pl.virtual_points) // pl.num_buckets, pl.num_windows * pl.num_buckets
