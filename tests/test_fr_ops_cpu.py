"""The BN254 scalar field Fr on raw limb records without a GPU: the hook msm_test_fr_raw_op lives in the hooks build only and its op numbers are
the Python constants; the integer model of tools/fr_ops_cases.py is cross-checked by plain arithmetic modulo r and its checker rejects what it
exists to catch; and tools/fr_bounds_check.cpp -- the host compile of csrc/fr_bn254.hpp with -DFP_BOUNDS_CHECK -- runs every operand class that
tests/test_gpu_22_fr_ops.py hands the device, fires no assertion and returns the model's limbs, limb for limb.  The negative control runs the same
program in a child process on the one illegal product (2^261 - 1)^2, which the header's former contract allowed: it must abort in fr_mul."""
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import mopro_msm_hip as mh
from mopro_msm_hip import testhooks as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fr_ops_cases as fc  # noqa: E402

R = fc.R
HIPCC = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"  # what csrc/Makefile builds the product with
SIZES = (1, 63, 64, 65)


# ---- the hook's place in the two builds, its constants and its wrapper -----------------------------------------------------------------------
def test_raw_hook_lives_in_the_hooks_build_only():
    assert "msm_test_fr_raw_op" in th.HOOK_SYMBOLS
    assert hasattr(th.load_hooks_library(), "msm_test_fr_raw_op") and not hasattr(mh.load_library(), "msm_test_fr_raw_op")
    assert "msm_test_fr_raw_op" not in open(os.path.join(ROOT, "include", "msm_hip.h")).read()
    assert "msm_test_fr_raw_op" not in mh.ABI_SYMBOLS


def test_header_defines_match_the_python_constants():
    hdr = open(os.path.join(ROOT, "include", "msm_hip_testhooks.h")).read()
    found = dict(re.findall(r"#define MSM_OP_FR_RAW_(\w+) (\d+)u\b", hdr))
    assert sorted(found) == sorted(fc.OPS) and th.FR_RAW_OPS == fc.OPS
    for i, name in enumerate(fc.OPS):
        assert int(found[name]) == i == getattr(th, "OP_FR_RAW_" + name) == getattr(fc, name), name
    assert tuple(th.FR_RAW_NEEDS_B) == tuple(fc.NEEDS_B)


def test_raw_hook_refuses_a_null_context():
    lib = th.load_hooks_library()
    a, b, out = np.zeros((1, 9), np.uint32), np.zeros((1, 9), np.uint32), np.zeros((1, 9), np.uint32)
    for op in range(len(fc.OPS)):
        assert lib.msm_test_fr_raw_op(None, op, mh._p32(a), mh._p32(b), mh._p32(out), 1) == mh.ERR_BAD_ARG
    assert not out.any()


def test_raw_wrapper_checks_shapes_before_the_call():
    """a missing or shorter b would let the C hook read past the buffer: the wrapper raises before it calls (no context is touched)"""
    call = th.HooksContext.test_fr_raw_op
    a = np.zeros((3, 9), np.uint32)
    for op in fc.NEEDS_B:
        with pytest.raises(ValueError):
            call(None, op, a, None)
        with pytest.raises(ValueError):
            call(None, op, a, np.zeros((2, 9), np.uint32))  # one record short
    with pytest.raises(ValueError):
        call(None, fc.MUL, a, np.zeros((3, 8), np.uint32))   # 24 words: not a whole number of 9-word records
    with pytest.raises(ValueError):
        call(None, len(fc.OPS), a, a)
    with pytest.raises(ValueError):
        call(None, fc.INV, np.zeros(8, np.uint32))           # not a whole record


# ---- the model -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def launches():
    """[(name, op, a, b)]: every launch the device test makes -- the random classes at every size, each edge class, the round trips and the twelve
    levels of the butterfly chain (fed forward by the model: the outputs are asserted equal to it, so these are the operands the device feeds back)"""
    rnd = random.Random(0xF2)
    out = []
    for op in range(len(fc.OPS)):
        for n in SIZES:
            a, b = fc.random_launch(op, n, rnd)
            out.append(("random %s n=%d" % (fc.OPS[op], n), op, a, b))
    for name, (op, a, b) in fc.edge_classes(rnd).items():
        out.append((name, op, a, b))
    run = lambda op, a, b: [fc.model(op, x, y) for x, y in zip(a, b)]

    def recording(op, a, b):
        out.append(("chain %s" % fc.OPS[op], op, a, b))
        return run(op, a, b)

    u, v, tw = fc.chain_start(rnd, 8)
    for s in range(fc.CHAIN_LEVELS):
        u, v = fc.chain_level(recording, s, u, v, tw[s])
    assert max(fc.value(x) for x in u + v) > 2 * R  # the chain did leave the reduced range
    return out


def test_tables_and_builders():
    fc.check_tables()
    assert fc.value(fc.rep(1)) == fc.R261 % R and fc.value(fc.rep(R - 1)) == (R - 1) * fc.R261 % R and fc.rep(0) == [0] * 9
    assert fc.limbs(fc.value([fc.MASK] * 9)) == [fc.MASK] * 9 and fc.value32(fc.words8(fc.R256 - 1)) == fc.R256 - 1
    rnd = random.Random(5)
    for _ in range(50):
        ls = fc.limbs(rnd.randrange(fc.R261))
        fat = fc.fatten(ls, rnd)
        assert fc.value(fat) == fc.value(ls) and fc.model(fc.NORMALIZE, fat) == ls
    # the header's former contract ("inputs normalised") is not enough; the corrected one is, and 168.78 r is inside it
    assert not fc.is_legal(fc.MUL, fc.limbs(fc.R261 - 1), fc.limbs(fc.R261 - 1))
    with pytest.raises(AssertionError):
        fc.mont(fc.R261 - 1, fc.R261 - 1)
    assert ((fc.R261 - 1) ** 2 + (fc.R261 - 1) * R) >> 261 >= fc.R261  # with m at its largest the top limb does leave 29 bits
    lim = 16878 * R // 100
    assert lim * lim < fc.MUL_LIMIT and fc.is_legal(fc.MUL, fc.limbs(lim), fc.limbs(lim))
    # the legality checks refuse what the header forbids
    assert not fc.is_legal(fc.ADD, fc.limbs(fc.R261 - 1), fc.limbs(1))
    assert not fc.is_legal(fc.SUB3, fc.limbs(0), fc.limbs(2 * R)) and fc.is_legal(fc.SUB3, fc.limbs(0), fc.limbs(2 * R - 1))
    assert not fc.is_legal(fc.SUB2, fc.limbs(fc.R261 - 2 * R), fc.limbs(0)) and fc.is_legal(fc.SUB2, fc.limbs(fc.R261 - 2 * R - 1), fc.limbs(0))
    assert not fc.is_legal(fc.REDUCE_LT2R, fc.limbs(2 * R)) and not fc.is_legal(fc.PACK, fc.limbs(fc.R256))
    assert not fc.is_legal(fc.NORMALIZE, [0xFFFFFFFF] * 9) and not fc.is_legal(fc.MUL, [1 << 29] + [0] * 8, fc.limbs(1))
    assert not fc.is_legal(fc.INV, fc.limbs(fc.POW_LIMIT * R)) and not fc.is_legal(fc.POW_U32, fc.limbs(fc.POW_LIMIT * R), [3] + [0] * 8)


def test_model_agrees_with_plain_arithmetic_on_every_class(launches):
    """check_output compares the model's integer with x * y * 2^-261 mod r (and its kin), computed without the Montgomery model, and with the
    documented bound, for every element of every launch: the model itself is cross-checked here"""
    seen, elements = set(), 0
    for name, op, a, b in launches:
        out = [fc.model(op, a[i], b[i] if b is not None else None) for i in range(len(a))]
        fc.check_all(op, a, b, out, name)
        seen.add(op)
        elements += len(a)
    assert seen == set(range(len(fc.OPS))) and elements > 5000
    # the product scan's m is the model's: all limbs 2^29 - 1 in the class built for it
    op, a, b = fc.edge_classes(random.Random(1))["mul with m all ones"]
    assert all(fc.limbs(fc.mont_m(fc.value(x), fc.value(y))) == [fc.MASK] * 9 for x, y in zip(a, b))
    # round trips
    for w in fc.roundtrip_patterns(random.Random(2)):
        assert fc.model(fc.PACK, fc.model(fc.UNPACK, w)) == w
        assert fc.value32(fc.model(fc.TO_STD, fc.model(fc.FROM_STD, w))) == fc.value32(w) % R
    # a * inv(a) = rep(1)
    for v in (fc.R261 % R, 5, R - 1, 83 * R + 12345):
        prod = fc.model(fc.MUL, fc.limbs(v), fc.model(fc.INV, fc.limbs(v)))
        assert fc.value(prod) % R == fc.R261 % R


def test_check_output_rejects_what_it_exists_to_catch():
    rnd = random.Random(9)
    a, b = fc.limbs(rnd.randrange(84 * R)), fc.limbs(rnd.randrange(84 * R))
    good = fc.model(fc.MUL, a, b)
    fc.check_output(fc.MUL, a, b, good)
    rejected = {"value + r": fc.limbs(fc.value(good) + R), "one limb off": [good[0] ^ 1] + good[1:], "top limb off": good[:8] + [good[8] + 1]}
    carry = list(good)  # the same integer, one limb at 2^29 or more
    i = next(k for k in range(8) if carry[k + 1] > 0)
    carry[i] += 1 << 29
    carry[i + 1] -= 1
    assert fc.value(carry) == fc.value(good)
    rejected["not normalised"] = carry
    for what, bad in rejected.items():
        with pytest.raises(AssertionError):
            fc.check_output(fc.MUL, a, b, bad, what)
    x = fc.limbs(R + 5)
    for bad in (fc.limbs(R + 5), fc.limbs(6), fc.limbs(4)):          # not reduced; reduced wrongly
        with pytest.raises(AssertionError):
            fc.check_output(fc.REDUCE_LT2R, x, None, bad)
    fc.check_output(fc.REDUCE_LT2R, x, None, fc.limbs(5))
    w = fc.words8(rnd.getrandbits(256))
    un = fc.model(fc.UNPACK, w)
    for k in range(9):                                               # a bit moved to the wrong limb
        bad = list(un)
        bad[k] ^= 1 << 28
        with pytest.raises(AssertionError):
            fc.check_output(fc.UNPACK, w, None, bad)
    packed = fc.model(fc.PACK, un)
    assert packed == w[:8] + [0]
    with pytest.raises(AssertionError):
        fc.check_output(fc.PACK, un, None, packed[:8] + [1])         # word 8 must be written as 0
    with pytest.raises(AssertionError):
        fc.check_output(fc.SUB3, a, fc.limbs(R), fc.limbs(fc.value(a) + 2 * R - R))  # a + 2r - b for a + 3r - b: a wrong pad row
    with pytest.raises(AssertionError):
        fc.check_all(fc.MUL, [a], [b], [good, good])
    with pytest.raises(AssertionError):                              # an illegal operand is refused by the model, whatever the output
        fc.check_output(fc.MUL, fc.limbs(fc.R261 - 1), fc.limbs(fc.R261 - 1), good)


# ---- the host compile of fr_bn254.hpp, every assertion live ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("fr_bounds_check")
    exe = d / "fr_bounds_check"
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-DFP_BOUNDS_CHECK", "-x", "hip", "--cuda-host-only",  # host code only: no device pass
                    os.path.join(ROOT, "tools", "fr_bounds_check.cpp"), "-o", str(exe)], check=True, capture_output=True, timeout=900)
    return d, exe


def write_launches(path, items):
    flat = []
    for _, op, a, b in items:
        flat += fc.launch_words(op, a, b)
    np.array(flat, np.uint32).tofile(path)


def test_host_run_fires_no_assertion_and_returns_the_models_limbs(driver, launches):
    d, exe = driver
    fin, fout = d / "in.bin", d / "out.bin"
    write_launches(fin, launches)
    r = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    elements = sum(len(a) for _, _, a, _ in launches)
    assert r.stdout.strip().split("\n")[-1] == "%d launches, %d elements, no bound violated" % (len(launches), elements)
    got = np.fromfile(fout, np.uint32).reshape(-1, 9)
    assert len(got) == elements
    at = 0
    for name, op, a, b in launches:
        fc.check_all(op, a, b, got[at:at + len(a)], name)  # every element of every launch
        at += len(a)


def test_negative_control_the_illegal_square_aborts_in_fr_mul(driver):
    """(2^261 - 1)^2: both operands normalised, the product outside A * B < (2^261 - r) * 2^261.  The host program, in a child process of its own,
    must die on the assertion in fr_mul: the assertions are compiled in, and the former contract was false.  A CPU program only: nothing illegal
    is ever handed to the device hook"""
    d, exe = driver
    fin, fout = d / "illegal.bin", d / "illegal_out.bin"
    write_launches(fin, [("illegal",) + fc.ILLEGAL_MUL])
    r = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "fr_mul: result not normalised" in r.stderr, (r.returncode, r.stdout, r.stderr)
    assert "no bound violated" not in r.stdout and not fout.exists()
    # the largest legal square beside it passes
    write_launches(fin, [("legal",) + fc.edge_classes(random.Random(1))["mul top of the domain"]])
    r = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "no bound violated" in r.stdout, r.stderr
