"""The state a context carries from one call to the next (-m gpu): first calls on fresh contexts and calls that follow an unfinished or refused one, on
every MSM entry point.

What differs between a fresh and a warm context is msm_ctx::flags_clean -- "the device flag words are known to be zero".  A context not known clean
(never used, or left by a call that ended before its results were collected) has its flag words zeroed from the host, and a struct-array call
(msm_arkworks) raises error bit 16 in those words from k_ark_repack when a struct has its `infinity` byte set: the call is then repeated with the
flags as a mask.  A zeroing that is ordered behind the repack erases the bit; the identity structs' (0, 0) words are then accumulated as points and
the call returns MSM_OK with a wrong point.  Every other test of the suite reaches its interesting input on a context that has completed a call.

Every case creates its own context.  Every comparison is word-exact against a reference that does not come from the code under test: the committed
goldens, the closed form (bases k_i * G from the oracle, expected (sum of k_i s_i over the points that count) * G by the oracle's scalar
multiplication) and, for G2, the Python law of tools/bn254_g2_py.py.  Sizes are the smallest that select the branch of the host path: 64 / 4095 (bases on
the compute stream), 4096 / 4097 (bases on the copy stream), 4097 with stage timing (compute stream again), 1024 in chunks of 2^8 (streamed).

Bit 1 ("a scalar is >= 2^254") and the struct entry: msm_arkworks takes Fr MONTGOMERY words, and k_decompose* / k_decompose_glv* convert them first
(fr_from_mont: a full Montgomery reduction with its final subtraction, so any 256-bit pattern comes out below r < 2^254) and test bit 254 of the
CONVERTED value.  The check therefore cannot fire through that entry: there is no struct call "with a bad scalar" that reports ERR_BAD_ARG.  What the
entry does with such words is tested instead (test_struct_entry_reduces_any_scalar_words): they count as their value times 2^-256 mod r.

Against the runtime as it was before flags_begin (msm_hip.hip), on an MI355X, 23 of the 94 cases returned a wrong point and 71 passed: every flagged
first call whose bases travel on the compute stream (n = 64, 4095, and 4097 with stage timing: both plans, both libraries, and the golden), the flagged
struct call after either abandoned call, after a refused layout and with arbitrary scalar words, and the hooks sequence at its first
"abandon -> flagged structs" step.  The copy-stream sizes (4096, 4097), the streamed shapes, every case without flags, every other entry point after an
abandoned call, every bit-1 case and the product sequence (its first flagged struct call comes on a warm context) passed there too.  The whole file runs
in about 3 seconds."""
import functools
import os
import random
import sys

import numpy as np
import pytest

import mopro_msm_hip as mh
from mopro_msm_hip import testhooks as th
from conftest import ROOT, load_golden
from oracle import bn254_oracle as orc

sys.path.insert(0, os.path.join(ROOT, "tools"))
import bn254_g2_py as g2  # noqa: E402
from ark_cases import ark_image, ark_image_of_mont_words, fr_mont  # noqa: E402

pytestmark = pytest.mark.gpu

R = orc.R_ORDER
RINV = pow(1 << 256, -1, R)
LAYOUT = (72, 0, 32, 64)
NMAX = 4400  # points of the shared synthetic instance: 4097 and room for the sequence's offsets
G2_A0, G2_D0 = 0x1234567890ABCDEF1234567890ABCDEF, 0xFEDCBA987654321
BAD_BIT = np.uint32(0x40000000)  # bit 254 of a scalar: word 7, bit 30
LIBS = {"product": mh.MsmContext, "hooks": th.HooksContext}
PLANS = {"default": {}, "noglv_c13": {"flags": mh.FLAG_NO_GLV, "window_bits": 13}}  # the second: no phi records behind the repacked words


# ---- references, computed once and never written to again ----------------------------------------------------------------------
def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def g1_instance():
    """(k, s, bases as arkworks Montgomery words, bases in standard form): P_i = k_i * G, k_i != 0"""
    k = orc.gen_scalars(0xB2542101, NMAX, nonzero=True)
    s = orc.gen_scalars(0xB2542102, NMAX, nonzero=True)
    return _frozen(k), _frozen(s), _frozen(orc.gen_bases_from_logs(k, orc.FORM_MONT)), _frozen(orc.gen_bases_from_logs(k, orc.FORM_STD))


@functools.lru_cache(maxsize=None)
def g2_instance():
    """standard-form words of Q_i = (G2_A0 + i * G2_D0) * G2, i < NMAX"""
    return _frozen(np.array([g2.point_words(p) for p in g2.chain_points(G2_A0, G2_D0, NMAX)], np.uint32))


def expect_g1(k, s, keep=None, mont_scalars=False):
    """(affine standard-form words, is_infinity) of sum_i s_i k_i G over the rows of `keep`; mont_scalars: s_i are Montgomery words of s_i * 2^-256"""
    if keep is not None:
        k, s = k[keep], s[keep]
    tot = orc.dot_words(k, s) * (RINV if mont_scalars else 1) % R
    gen = np.zeros(16, np.uint32)
    gen[0], gen[8] = 1, 2
    aff, inf = orc.g1_to_affine_std(orc.g1_scalar_mul(gen, orc.int_to_words(tot)))
    return aff, bool(inf)


def expect_g2(s, lo, keep=None):
    """the same for the G2 instance rows lo .. lo + len(s): (32 words, is_infinity)"""
    ints = [orc.words_to_int(row) for row in s]
    tot = sum(v * (G2_A0 + (lo + i) * G2_D0) for i, v in enumerate(ints) if keep is None or keep[i]) % R
    pt = g2.mul(g2.G2_GEN, tot)
    return np.array(g2.affine_words_std(pt), np.uint32), pt is None


def check(r, exp, what):
    words, inf = exp
    assert r.is_infinity == inf, (what, "is_infinity", r.is_infinity)
    if not inf:
        assert (r.affine_std == words).all(), (what, "the result differs from the reference")


def with_bad_scalar(s, i):
    bad = np.array(s, np.uint32)
    bad[i, 7] |= BAD_BIT
    assert orc.words_to_int(bad[i]) >= 1 << 254
    return bad


def struct_call(c, img, scalars_mont):
    return c.msm_arkworks(img, *LAYOUT, scalars_mont)


def to_dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.uint32).view(np.int32).reshape(-1)).to("cuda:0")  # (a copy: the shared references are read-only)


def mask_to_dev(inf):
    import torch
    return torch.from_numpy(np.array(inf, dtype=np.uint8)).to("cuda:0")


def device_call(c, bases_mont, scalars, inf=None):
    import torch
    d_b, d_s = to_dev(bases_mont), to_dev(scalars)
    d_i = mask_to_dev(inf) if inf is not None else None
    torch.cuda.synchronize()
    return c.msm_device(d_b.data_ptr(), d_s.data_ptr(), scalars.shape[0], d_inf_ptr=d_i.data_ptr() if d_i is not None else None)


def golden_struct_case():
    """tests/golden/msm_edge_inf_bases.npz as a struct array: 64 points, 3 flagged, each with a non-zero scalar (an accumulated (0, 0) cannot cancel)"""
    g = load_golden("edge_inf_bases")
    flagged = np.flatnonzero(g["inf"])
    assert g["bases"].shape[0] == 64 and len(flagged) == 3 and g["scalars"][flagged].any(axis=1).all() and not g["expected_inf"]
    img = ark_image(g["bases"], g["inf"], *LAYOUT, np.random.default_rng(21))
    return img, fr_mont(g["scalars"]), (g["expected"], False)


# ---- A. first call on a fresh context: a struct array with `infinity` flags set ---------------------------------------------------
# (id, points, stream_chunk_log2, stage timing, flagged positions)
BRANCHES = [
    ("n64_compute_stream", 64, 0, False, (0, 31, 63)),
    ("n4095_compute_stream", 4095, 0, False, (0, 2047, 4094)),
    ("n4096_copy_stream", 4096, 0, False, (0, 2048, 4095)),
    ("n4097_copy_stream", 4097, 0, False, (0, 2048, 4096)),
    ("n4097_stage_timing", 4097, 0, True, (0, 2048, 4096)),
    ("n1024_streamed_flags_in_chunk_0", 1024, 8, False, (3, 100)),
    ("n1024_streamed_flags_in_last_chunk", 1024, 8, False, (768, 1023)),
    ("n1024_streamed_flags_on_a_chunk_boundary", 1024, 8, False, (255, 256)),
]


@pytest.mark.parametrize("flagged", [True, False], ids=["flags_set", "no_flags"])
@pytest.mark.parametrize("lib", list(LIBS))
@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("branch", BRANCHES, ids=[b[0] for b in BRANCHES])
def test_first_struct_call_on_a_fresh_context(branch, plan, lib, flagged):
    _, n, chunk_log2, timing, positions = branch
    k, s, bases, _ = g1_instance()
    k, s, bases = k[:n], s[:n], bases[:n]
    inf = np.zeros(n, np.uint8)
    if flagged:
        inf[list(positions)] = 1
        assert s[list(positions)].any(axis=1).all(), "a flagged position carries a zero scalar: its (0, 0) record could not show"
    img = ark_image_of_mont_words(bases, inf, np.random.default_rng(n))
    exp = expect_g1(k, s, inf == 0, mont_scalars=True)  # (s handed over as Montgomery words: it counts as s * 2^-256)
    assert not exp[1]
    with LIBS[lib](stream_chunk_log2=chunk_log2, **PLANS[plan]) as c:
        if timing:
            c.set_stage_timing(True)
        first = struct_call(c, img, s)
        assert c.timings()["stream_chunks"] == (4 if chunk_log2 else 0)  # the branch this case is named after
        check(first, exp, "first call on the fresh context")
        again = struct_call(c, img, s)
        check(again, exp, "the same call on the now warm context")
        assert (again.affine_std == first.affine_std).all()


@pytest.mark.parametrize("lib", list(LIBS))
@pytest.mark.parametrize("plan", list(PLANS))
def test_first_struct_call_on_a_fresh_context_golden(plan, lib):
    img, sm, exp = golden_struct_case()
    with LIBS[lib](**PLANS[plan]) as c:
        first = struct_call(c, img, sm)
        check(first, exp, "first call on the fresh context")
        again = struct_call(c, img, sm)
        check(again, exp, "the same call on the now warm context")
        assert (again.affine_std == first.affine_std).all()


# ---- B. first call after an unfinished call ---------------------------------------------------------------------------------------
def abandon(c, bad):
    """a call that ends between its sort and its accumulation: flags_clean stays false, the list counters stay dirty -- and with a scalar >= 2^254
    error bit 1 stays raised on the device, never collected"""
    sc = load_golden("rand_n256")["scalars"]
    if bad:
        sc = with_bad_scalar(sc, 200)
    with pytest.raises(mh.MsmError) as e:
        c.abandon_after_sort(sc)
    assert e.value.code == mh.ERR_HIP


def follow_arkworks(c):
    img, sm, exp = golden_struct_case()
    for what in ("first call after the unfinished one", "repeated"):
        check(struct_call(c, img, sm), exp, what)


def follow_msm(c):
    g = load_golden("rand_n256")
    for what in ("first call after the unfinished one", "repeated"):
        check(c.msm(g["bases"], g["scalars"], mh.FORM_STD, g["inf"]), (g["expected"], bool(g["expected_inf"])), what)


def follow_device(c):
    k, s, bases, _ = g1_instance()
    n = 64
    inf = np.zeros(n, np.uint8)
    inf[[0, 31, 63]] = 1
    exp = expect_g1(k[:n], s[:n], inf == 0)
    for what in ("first call after the unfinished one", "repeated"):
        check(device_call(c, bases[:n], s[:n], inf), exp, what)


def follow_g2(c):
    g = np.load(os.path.join(ROOT, "tests", "golden", "msm_g2_rand_n17.npz"))
    for what in ("first call after the unfinished one", "repeated"):
        r = c.msm_g2(g["bases"], g["scalars"], mh.FORM_STD, g["inf"] if g["inf"].any() else None)
        check(r, (g["expected"], bool(g["expected_inf"])), what)


def follow_resident(c):
    g = load_golden("rand_n256")
    c.upload_bases(g["bases"], mh.FORM_STD, g["inf"])
    for what in ("first call after the unfinished one", "repeated"):
        check(c.msm_resident(g["scalars"]), (g["expected"], bool(g["expected_inf"])), what)


FOLLOW = {"arkworks_flagged": follow_arkworks, "msm": follow_msm, "device_inf_mask": follow_device, "g2": follow_g2, "resident": follow_resident}


@pytest.mark.parametrize("bad", [False, True], ids=["good_scalars", "scalar_above_2_254"])
@pytest.mark.parametrize("follow", list(FOLLOW))
def test_first_call_after_an_unfinished_call(follow, bad):
    """no stale bit may reach the next call (ERR_BAD_ARG from the abandoned call's scalar, "unexpected error bit 16" on G2), and the next call's own
    bit 16 must survive the clean-up"""
    with th.HooksContext() as c:
        abandon(c, bad)
        FOLLOW[follow](c)


@pytest.mark.parametrize("lib", list(LIBS))
def test_a_host_side_refusal_leaves_a_fresh_context_fresh(lib):
    """a struct layout refused before any kernel (ERR_BAD_ARG) on a fresh context: the flagged struct call that follows is still a first call"""
    img, sm, exp = golden_struct_case()
    with LIBS[lib]() as c:
        with pytest.raises(mh.MsmError) as e:
            c.msm_arkworks(img, 72, 2, 32, 64, sm)
        assert e.value.code == mh.ERR_BAD_ARG
        check(struct_call(c, img, sm), exp, "first call after the refusal")
        check(struct_call(c, img, sm), exp, "repeated")


# ---- C. first call that raises bit 1 ----------------------------------------------------------------------------------------------
def bit1_msm(c, n=64):
    """(the call as a function of the scalars, good scalars, the reference for them)"""
    k, s, bases, _ = g1_instance()
    return (lambda sc: c.msm(bases[:n], sc, mh.FORM_MONT)), s[:n], expect_g1(k[:n], s[:n])


def bit1_msm_streamed(c):
    return bit1_msm(c, 1024)  # four chunks of 2^8


def bit1_device(c, n=64):
    k, s, bases, _ = g1_instance()
    return (lambda sc: device_call(c, bases[:n], sc)), s[:n], expect_g1(k[:n], s[:n])


def bit1_g2(c):
    g = np.load(os.path.join(ROOT, "tests", "golden", "msm_g2_rand_n17.npz"))
    inf = g["inf"] if g["inf"].any() else None
    return (lambda sc: c.msm_g2(g["bases"], sc, mh.FORM_STD, inf)), g["scalars"], (g["expected"], bool(g["expected_inf"]))


def bit1_resident(c, n=64):
    k, s, bases, _ = g1_instance()
    c.upload_bases(bases[:n], mh.FORM_MONT)
    return (lambda sc: c.msm_resident(sc)), s[:n], expect_g1(k[:n], s[:n])


BIT1 = {"msm": bit1_msm, "msm_streamed": bit1_msm_streamed, "device": bit1_device, "g2": bit1_g2, "resident": bit1_resident}


@pytest.mark.parametrize("lib", list(LIBS))
@pytest.mark.parametrize("entry", list(BIT1))
def test_first_call_with_a_scalar_above_2_254(entry, lib):
    """the scalar sits at index n - 1 (streamed: in the last chunk only): ERR_BAD_ARG, and the next good call on the same context is word-exact; then
    the same pair on the warm context"""
    streamed = entry == "msm_streamed"
    with LIBS[lib](stream_chunk_log2=8 if streamed else 0) as c:
        call, good, exp = BIT1[entry](c)
        bad = with_bad_scalar(good, good.shape[0] - 1)
        for what in ("fresh", "warm"):
            with pytest.raises(mh.MsmError) as e:
                call(bad)
            assert e.value.code == mh.ERR_BAD_ARG, what
            check(call(good), exp, what + ": the good call after ERR_BAD_ARG")
            if entry.startswith("msm"):
                assert c.timings()["stream_chunks"] == (4 if streamed else 0)


@pytest.mark.parametrize("lib", list(LIBS))
def test_struct_entry_reduces_any_scalar_words(lib):
    """see the module docstring: the struct entry's scalars are Montgomery words, converted before bit 254 is looked at, so no word pattern raises bit 1
    there.  A flagged struct array whose last scalar is 2^256 - 1 (and one with bit 254 set), fresh and warm: the retry runs and the words count as
    their value * 2^-256 mod r -- which dot_words(k, s) * 2^-256 mod r is for ANY 256-bit s_i."""
    k, s, bases, _ = g1_instance()
    n = 64
    inf = np.zeros(n, np.uint8)
    inf[[0, 31]] = 1
    sc = with_bad_scalar(s[:n], 5)
    sc[n - 1] = 0xFFFFFFFF
    img = ark_image_of_mont_words(bases[:n], inf, np.random.default_rng(3))
    exp = expect_g1(k[:n], sc, inf == 0, mont_scalars=True)
    assert not exp[1]
    with LIBS[lib]() as c:
        check(struct_call(c, img, sc), exp, "fresh")
        check(struct_call(c, img, sc), exp, "warm")


# ---- D. a seeded sequence ------------------------------------------------------------------------------------------------------------
SEQ_SEED = 0x21C0DE
SEQ_SIZES = (1, 17, 64, 256, 4097)
SEQ_INPUTS = {
    "msm_std": ("clean", "inf_mask", "bad_scalar"),
    "msm_mont": ("clean", "inf_mask", "bad_scalar"),
    "arkworks": ("clean", "flagged"),  # (no bad scalar through this entry: module docstring)
    "device": ("clean", "inf_mask", "bad_scalar"),
    "g2": ("clean", "inf_mask", "bad_scalar"),
    "resident": ("clean", "inf_mask", "bad_scalar"),
    "abandon": ("clean", "bad_scalar"),  # hooks context only
}
# the transitions the sequence must contain: (entry or None, input or None) of a step and of the step behind it
FLAGGED = ("arkworks", "flagged")
SEQ_TRANSITIONS = {
    "abandon -> flagged structs": (("abandon", None), FLAGGED),
    "bad scalar -> flagged structs": ((None, "bad_scalar"), FLAGGED),
    "G2 -> flagged structs": (("g2", None), FLAGGED),
    "flagged structs -> G2": (FLAGGED, ("g2", None)),
}
SEQ_FORCED = [("abandon", "clean", 64), ("arkworks", "flagged", 64), ("msm_std", "bad_scalar", 17), ("arkworks", "flagged", 256),
              ("g2", "clean", 17), ("arkworks", "flagged", 4097), ("g2", "inf_mask", 64), ("abandon", "bad_scalar", 256), ("arkworks", "flagged", 17)]


def draw_sequence(seed, with_abandon):
    rng = random.Random(seed)
    drawn = []
    for _ in range(31):
        entry = rng.choice(list(SEQ_INPUTS))
        drawn.append((entry, rng.choice(SEQ_INPUTS[entry]), rng.choice(SEQ_SIZES)))
    at = rng.randrange(1, len(drawn))
    steps = drawn[:at] + SEQ_FORCED + drawn[at:]
    return steps if with_abandon else [st for st in steps if st[0] != "abandon"]


def _matches(step, pattern):
    return (pattern[0] is None or step[0] == pattern[0]) and (pattern[1] is None or step[1] == pattern[1])


def transitions_of(steps):
    return {name for name, (a, b) in SEQ_TRANSITIONS.items() if any(_matches(p, a) and _matches(q, b) for p, q in zip(steps, steps[1:]))}


def run_step(c, step, idx):
    """(what the context gave, what the reference says): each ("ok", is_infinity, words or None) or ("error", code)"""
    entry, kind, n = step
    K, S, BM, BS = g1_instance()
    lo = (idx * 37) % (NMAX - n + 1)
    k, s = K[lo:lo + n], S[lo:lo + n]
    masked = np.zeros(n, np.uint8)
    if kind in ("inf_mask", "flagged"):
        masked[sorted({0, n // 2, n - 1})] = 1  # (n = 1: every point -- the identity)
    inf = masked if kind in ("inf_mask", "flagged") else None
    sc = with_bad_scalar(s, n - 1) if kind == "bad_scalar" else s
    if entry == "abandon":
        want = ("error", mh.ERR_HIP)
    elif kind == "bad_scalar":
        want = ("error", mh.ERR_BAD_ARG)
    elif entry == "g2":
        words, is_inf = expect_g2(s, lo, masked == 0)
        want = ("ok", is_inf, None if is_inf else words.tobytes())
    else:
        words, is_inf = expect_g1(k, s, masked == 0, mont_scalars=entry == "arkworks")
        want = ("ok", is_inf, None if is_inf else words.tobytes())
    try:
        if entry == "abandon":
            c.abandon_after_sort(sc)
            return ("ok", None, None), want
        if entry == "msm_std":
            r = c.msm(BS[lo:lo + n], sc, mh.FORM_STD, inf)
        elif entry == "msm_mont":
            r = c.msm(BM[lo:lo + n], sc, mh.FORM_MONT, inf)
        elif entry == "arkworks":
            r = struct_call(c, ark_image_of_mont_words(BM[lo:lo + n], inf, np.random.default_rng(idx)), sc)
        elif entry == "device":
            r = device_call(c, BM[lo:lo + n], sc, inf)
        elif entry == "g2":
            r = c.msm_g2(g2_instance()[lo:lo + n], sc, mh.FORM_STD, inf)
        else:
            c.upload_bases(BM[lo:lo + n], mh.FORM_MONT, inf)
            r = c.msm_resident(sc)
    except mh.MsmError as e:
        return ("error", e.code), want
    return ("ok", bool(r.is_infinity), None if r.is_infinity else np.asarray(r.affine_std, np.uint32).tobytes()), want


@pytest.mark.parametrize("lib", ["hooks", "product"])
def test_seeded_sequence_of_calls_on_one_context(lib):
    """~40 steps drawn from a fixed seed on ONE context: entry point x input x size, every outcome (result words or error code) against the
    reference.  The product context has no abandon hook: its sequence is the same one without those steps."""
    steps = draw_sequence(SEQ_SEED, with_abandon=lib == "hooks")
    needed = set(SEQ_TRANSITIONS) if lib == "hooks" else set(SEQ_TRANSITIONS) - {"abandon -> flagged structs"}
    assert needed <= transitions_of(steps), (needed - transitions_of(steps), "missing from the sequence")
    assert len(draw_sequence(SEQ_SEED, True)) == 40 and len(steps) >= 30
    with LIBS[lib]() as c:
        prev = None
        for idx, step in enumerate(steps):
            got, want = run_step(c, step, idx)
            assert got == want, (f"seed {SEQ_SEED:#x} step {idx} {step} after {prev}: the context gave {got[:2]}, the reference says {want[:2]}"
                                 + ("" if got[:2] != want[:2] else " (the words differ)"))
            prev = step
