"""What the MSM case builders of both groups share (tools/g1_msm_cases.py, tools/g2_msm_cases.py): the index logic of an instance whose bases have
known logarithms, the seeded and the digit-disjoint scalars, the bucket sizes of an unsplit plan with plain digits, and the piece rule of the
accumulation written down once more in Python integers -- make_piece_plan, effective_pmax and effective_psplit of csrc/msm_planner.hpp
(tools/piece_plan_check.cpp runs the C++ for tests/test_g1_msm_cases_cpu.py to compare), decode_piece_lengths and piece_split of
csrc/msm_kernels.hpp (device functions: the device's list counters are their check) -- from which expected_lists gives the five counters of
HooksContext.list_counts().  Nothing here touches the code under test."""
import math
import random
from collections import Counter

import numpy as np

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
FORM_STD, FORM_MONT = 0, 1
FLAG_UNSIGNED_DIGITS, FLAG_NO_GLV = 1, 2  # MSM_FLAG_* of include/msm_hip.h


def scalar_words(vs):
    return np.array([[(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)] for v in vs], np.uint32).reshape(len(vs), 8)


class Instance:
    """rows (point upts[pidx[i]] of logarithm ulogs[pidx[i]], scalar uscal[sidx[i]]), row i masked as infinity where inf[i]; zeroed[i]: the
    masked row's base words are zeros instead of the point's.  A group's module derives it with point_words (the words of upts in a form) and
    product (total * generator as that module spells an expected value, None for the identity)."""

    def __init__(self, ulogs, upts, pidx, uscal, sidx, inf=None, zeroed=None):
        self.ulogs, self.upts, self.uscal = [c % R for c in ulogs], list(upts), [s % R for s in uscal]
        self.pidx, self.sidx = np.asarray(pidx, np.int64), np.asarray(sidx, np.int64)
        assert len(self.pidx) == len(self.sidx) and len(self.ulogs) == len(self.upts)
        self.inf = None if inf is None else np.asarray(inf, np.uint8)
        self.zeroed = zeroed
        self._expected = None

    def point_words(self, form):
        raise NotImplementedError

    def product(self, total):
        raise NotImplementedError

    @property
    def n(self):
        return len(self.pidx)

    def scalars(self):
        return [self.uscal[j] for j in self.sidx.tolist()]

    def logs(self):
        return [self.ulogs[j] for j in self.pidx.tolist()]

    def total(self):
        live = [True] * self.n if self.inf is None else [not m for m in self.inf.tolist()]
        return sum(self.uscal[s] * self.ulogs[p] for p, s, ok in zip(self.pidx.tolist(), self.sidx.tolist(), live) if ok) % R

    def expected(self):
        if self._expected is None:
            self._expected = (self.product(self.total()),)  # (None for 0; one scalar multiplication, made once)
        return self._expected[0]

    def emit(self, form=FORM_MONT):
        bases = np.ascontiguousarray(self.point_words(form)[self.pidx])
        if self.zeroed is not None:
            bases[np.asarray(self.zeroed, bool)] = 0
        return bases, np.ascontiguousarray(scalar_words(self.uscal)[self.sidx]), self.inf, self.expected()


def seeded_scalars(seed, count):
    rnd = random.Random(seed ^ 0x5CA1A25)
    return [rnd.randrange(1, R) for _ in range(count)]


SPREAD_BITS = 234  # 254 - 20: below the top window of every window width the planner accepts


def spread_scalars(seed):
    """three scalars below 2^234 whose pairwise differences (XOR) have no two neighbouring zero bits below bit 234: s, s ^ 0101..., s ^ 1010...
    (bit 233 of s is zero).  Cut into windows of any width from 2 to 20 with plain digits, no two of them share a nonzero digit in any window, and
    the top window (the bits from c (W - 1) >= 234 on, whose entries the plan spreads over its buckets by point index) stays empty: every
    non-empty bucket of an instance tiled from them holds exactly T entries, whatever width the planner picks."""
    s = random.Random(seed ^ 0x5B8EAD).getrandbits(SPREAD_BITS - 1)
    m1 = sum(1 << b for b in range(0, SPREAD_BITS, 2))
    m2 = sum(1 << b for b in range(1, SPREAD_BITS, 2))
    return [s, s ^ m1, s ^ m2]


def mask_rows(inst, seed):
    """(inf, zeroed, uscal, sidx) of `inst` with about a quarter of its rows masked as infinity (every other one of them with zeroed base words, as a
    caller that keeps no coordinates for such a point would pass them) and about a sixth carrying the scalar 0; at least one row of each kind, and
    one row left alone"""
    rnd = random.Random(seed ^ 0x3A5C)
    n = inst.n
    assert n >= 3
    inf, sidx = np.zeros(n, np.uint8), inst.sidx.copy()
    uscal = inst.uscal + [0]
    for i in range(n):
        u = rnd.random()
        if u < 0.25:
            inf[i] = 1
        elif u < 0.42:
            sidx[i] = len(uscal) - 1
    order = rnd.sample(range(n), 3)
    inf[order[0]], inf[order[1]], inf[order[2]] = 1, 0, 0
    sidx[order[1]] = len(uscal) - 1
    sidx[order[2]] = inst.sidx[order[2]]
    masked = np.flatnonzero(inf)
    zeroed = np.zeros(n, bool)
    zeroed[masked[::2]] = True
    return inf, zeroed, uscal, sidx


# ---- which list a bucket reaches --------------------------------------------------------------------------------------------------------------
LONG_SPAN, LONG_SEG = 8, 1024  # pieces from which a bucket is folded by workgroups; pieces per workgroup (one segment)
PIECE_BINS_MAX, SPLIT_PIECES_TARGET, SPLIT_ENTRIES_SHIFT, SPARSE_BUCKETS_MAX = 1024, 1 << 18, 17, 65536  # csrc/msm_planner.hpp


def unsigned_bucket_sizes(scalars, inf, window_bits, scalar_bits=254):
    """entries per non-empty bucket of an unsplit plan with plain digits: digit w of s is (s >> (w * c)) & (2^c - 1), a zero digit and a masked
    row give no entry.  A Counter {(window, digit): entries}.  The TOP window's entries are spread over its buckets by point index (msm_plan_t
    top_digit_bits): instances whose buckets are counted leave it empty (spread_scalars, one_base_ramp), anything else is a ValueError."""
    c, sizes = window_bits, Counter()
    W = (scalar_bits + c - 1) // c
    for i, s in enumerate(scalars):
        if inf is not None and inf[i]:
            continue
        for w in range(W):
            d = (s >> (w * c)) & ((1 << c) - 1)
            if d and w == W - 1:
                raise ValueError("scalar %d has a digit in the top window" % i)
            if d:
                sizes[(w, d)] += 1
    return sizes


def make_piece_plan(pairs, mean_occupancy, total_buckets, forced_len=0, split_target=SPLIT_PIECES_TARGET):
    """(pmax, psplit) of msmplan::make_piece_plan for the first (or only) chunk of an instance"""
    pmax = min(PIECE_BINS_MAX, mean_occupancy + max(8, math.isqrt(4 * mean_occupancy)))
    if total_buckets < 1 << 17:
        pmax = min(pmax, max(8, pairs >> 17))
    want = min(pmax, max(8, (pairs + split_target - 1) // split_target))
    psplit = 8
    while psplit * 2 <= want:
        psplit *= 2
    if forced_len:
        pmax = psplit = min(forced_len, PIECE_BINS_MAX)
    return pmax, psplit


def effective_pmax(pmax, entries, nonempty):
    """msmplan::effective_pmax: the longest whole bucket as the device sees a SPARSE instance (never below the plan's)"""
    if nonempty == 0 or nonempty > SPARSE_BUCKETS_MAX:
        return pmax
    mean = min(entries // nonempty, 65536)
    two_sigma = math.isqrt(4 * mean)
    cand = mean + max(two_sigma, 8)
    cap = entries >> 16
    if mean >= 8 * cap:
        cap = max(cap, min(mean // 4, 32))
    cand = min(cand, cap, PIECE_BINS_MAX)
    return max(cand, pmax)


def effective_psplit(psplit, shift, entries):
    """msmplan::effective_psplit: the run length of very long buckets, shortened for instances that sort few entries (shift 0: never)"""
    want = entries >> shift
    p = 8
    while p * 2 <= want and p * 2 <= psplit:
        p *= 2
    return min(p, psplit)


def decode_piece_lengths(pmax, psplit, shift, fixed, entries, nonempty):
    """msmk::decode_piece_lengths: (pmax, run, equal) for THIS instance from the plan's lengths; fixed: a forced length, taken as it is;
    equal: pmax was raised, buckets up to LONG_SPAN x pmax are cut into equal runs (PSPLIT_EQUAL)"""
    run, equal = psplit & 0xFFFF, False
    if not fixed:
        raised = effective_pmax(pmax, entries, nonempty)
        run = effective_psplit(run, shift & 0xFF, entries)
        if raised > pmax:
            pmax, equal = raised, True
    return pmax, run, equal


def piece_split(sz, pmax, run, equal):
    """msmk::piece_split: (pieces m, entries q of pieces 0 .. m - 2; the last one holds the rest)"""
    if sz <= pmax:
        return 1, sz
    if sz > LONG_SPAN * pmax:
        q = run
    elif equal:
        m = (sz + pmax - 1) // pmax
        q = (sz + m - 1) // m
    else:
        q = pmax
    return (sz + q - 1) // q, q


def piece_branch(sz, pmax, run, equal):
    """the branch of piece_split a bucket takes: "whole", "psplit", "equal" or "pmax" """
    return "whole" if sz <= pmax else "psplit" if sz > LONG_SPAN * pmax else "equal" if equal else "pmax"


def device_lengths(piece_len=None, plan=None, entries=0, nonempty=0, shift=SPLIT_ENTRIES_SHIFT):
    """(pmax, run, equal) the kernels cut buckets by: a forced length (MSM_HIP_PIECE_LEN), or the unforced rule for `plan` = (pairs, mean occupancy,
    total buckets) of the host's plan and the entries / non-empty buckets the sort of this instance counts"""
    if piece_len:
        pmax, psplit = make_piece_plan(0, 0, 0, int(piece_len))
        return decode_piece_lengths(pmax, psplit, shift, True, entries, nonempty)
    pairs, mean, total_buckets = plan
    pmax, psplit = make_piece_plan(pairs, mean, total_buckets)
    return decode_piece_lengths(pmax, psplit, shift, False, entries, nonempty)


def expected_lists(sizes, piece_len=None, plan=None, entries=None, nonempty=None):
    """the list counters the piece rule leaves for buckets of these sizes.  A bucket cut into m > 1 pieces has a partial sum per piece; m = 2: the
    two-piece list, 3 .. 7: the mid list, 8 or more: the long list with one item per segment of 1024 pieces.  `pieces` counts every piece, those
    of whole buckets too.  piece_len: a forced length (a bucket of sz > piece_len entries is cut into ceil(sz / piece_len) pieces); otherwise
    plan = (pairs, mean occupancy, total buckets) and the unforced rule, with entries / nonempty as the device counts them (default: the sum and
    the number of `sizes`, what the two-level sort counts)."""
    sizes = list(sizes)
    if not piece_len:
        entries = sum(sizes) if entries is None else entries
        nonempty = sum(1 for sz in sizes if sz) if nonempty is None else nonempty
    pmax, run, equal = device_lengths(piece_len, plan, entries or 0, nonempty or 0)
    out = dict(long=0, mid=0, pieces=0, partials=0, mid2=0)
    for sz in sizes:
        m, _ = piece_split(sz, pmax, run, equal)
        out["pieces"] += m
        if m == 1:
            continue
        out["partials"] += m
        if m == 2:
            out["mid2"] += 1
        elif m < LONG_SPAN:
            out["mid"] += 1
        else:
            out["long"] += (m + LONG_SEG - 1) // LONG_SEG
    return out
