"""The BN254 base field Fq and Fq2 on raw limb records without a GPU: the hooks msm_test_fq_raw_op / msm_test_fq2_raw_op live in the hooks build
only, their op numbers are the Python constants and the pad multiples K they dispatch are exactly the instantiations of csrc/; the integer model of
tools/fq_ops_cases.py is cross-checked by plain arithmetic modulo p and its checker rejects what it exists to catch; and tools/fq_bounds_check.cpp
-- the host compile of csrc/fp_bn254.hpp and csrc/fp2_bn254.hpp with -DFP_BOUNDS_CHECK -- runs every launch that tests/test_gpu_24_fq_ops.py hands
the device, fires no assertion and returns the model's limbs, limb for limb.  The negative control runs the same program in a child process on
fp_mul_add of four operands of 128p, which the header's former contract allowed: it must abort on the assertion of the normalised result."""
import glob
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
CSRC = os.path.join(ROOT, "gpu-acceleration_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fq_ops_cases as fc  # noqa: E402

P = fc.P
HIPCC = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"  # what csrc/Makefile builds the product with
SIZES = (1, 63, 64, 65)
HOOKS = ("msm_test_fq_raw_op", "msm_test_fq2_raw_op")


# ---- the hooks' place in the two builds, their constants and their wrappers ------------------------------------------------------------------
def test_raw_hooks_live_in_the_hooks_build_only():
    hdr = open(os.path.join(ROOT, "include", "msm_hip.h")).read()
    for name in HOOKS:
        assert name in th.HOOK_SYMBOLS and name not in mh.ABI_SYMBOLS and name not in hdr
        assert hasattr(th.load_hooks_library(), name) and not hasattr(mh.load_library(), name)


def test_header_defines_match_the_python_constants():
    hdr = open(os.path.join(ROOT, "include", "msm_hip_testhooks.h")).read()
    for prefix, kinds, wrapper_kinds in (("FQ", fc.FQ_KINDS, th.FQ_RAW_KINDS), ("FQ2", fc.FQ2_KINDS, th.FQ2_RAW_KINDS)):
        found = dict(re.findall(r"#define MSM_OP_%s_RAW_(\w+) (\d+)u\b" % prefix, hdr))
        assert sorted(found) == sorted(kinds) and wrapper_kinds == kinds
        for i, name in enumerate(kinds):
            assert int(found[name]) == i, name
    assert th.FQ_RAW_ARITY == fc.FQ_ARITY and th.FQ_RAW_K == fc.FQ_K and th.FQ2_RAW_WORDS == fc.FQ2_WORDS and th.FQ2_RAW_K == fc.FQ2_K
    for op in fc.ALL_OPS:
        assert fc.op_word(op) == (th.fq_raw_op if op[0] == 1 else th.fq2_raw_op)(op[1], op[2])


def dispatched():
    """{(field, kind): set of K} the hook and the host program dispatch: the X-macro lists of csrc/msm_testhooks_fq_raw.hpp"""
    text = open(os.path.join(CSRC, "msm_testhooks_fq_raw.hpp")).read()
    out = {}
    for field, prefix in ((1, "FQ"), (2, "FQ2")):
        body = re.search(r"#define MSM_%s_RAW_OPS\(X\)(.*?)\n\n" % prefix, text, re.S).group(1)
        for kind, k in re.findall(r"X\(MSM_OP_%s_RAW_(\w+), (\d+)\)" % prefix, body):
            out.setdefault((field, kind), set()).add(int(k))
    return out


def test_pad_multiples_are_the_instantiations_of_the_sources():
    """every fp_sub<K>, fp_neg<K>, fp_neg_raw<K>, fp2_mul<K>, fp2_sqr<K>, fp2_sub<K>, fp2_neg<K>, g2_conj_mul<K> with a literal K in csrc/ outside
    the hooks files is dispatched by the hooks, and the hooks dispatch no other: a new instantiation without a test fails here"""
    found = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if os.path.basename(path).startswith("msm_testhooks") or not os.path.isfile(path):
            continue
        text = re.sub(r"//[^\n]*", "", open(path).read())  # the code, not what the comments quote
        for name, k in re.findall(r"\b(fp2?_(?:sub|neg|mul|sqr)(?:_raw)?|g2_conj_mul)<(\d+)>", text):
            found.setdefault(name, set()).add(int(k))
    assert found.pop("fp_sub_raw") == {8}  # the one raw subtraction: the Y3 kinds
    neg_raw = found.pop("fp_neg_raw")
    assert neg_raw == {2, 3, 4, 6} and neg_raw - {2, 4} == set(fc.FQ_K["Y3"])  # <2> and <4>: MUL_NEG_RAW2 / NORMALIZE_NEG_RAW2, SUB6_NEG_RAW4
    want = {(1, "SUB"): found.pop("fp_sub"), (1, "NEG"): found.pop("fp_neg"), (2, "MUL"): found.pop("fp2_mul"), (2, "SQR"): found.pop("fp2_sqr"),
            (2, "SUB"): found.pop("fp2_sub"), (2, "NEG"): found.pop("fp2_neg"), (2, "CONJ"): found.pop("g2_conj_mul"), (1, "Y3"): {3, 6}}
    assert not found, found
    got = dispatched()
    assert {key: ks for key, ks in got.items() if ks != {0}} == want
    assert {key: set(ks) for key, ks in list({(1, k): v for k, v in fc.FQ_K.items()}.items()) + list({(2, k): v for k, v in fc.FQ2_K.items()}.items())} == want
    assert sorted(got) == sorted({(op[0], op[1]) for op in fc.ALL_OPS}) and sum(len(v) for v in got.values()) == len(fc.ALL_OPS)
    # the sets as they stand today, spelled out
    assert want[1, "SUB"] == set(range(2, 9)) and want[1, "NEG"] == {2, 3, 4, 6} and want[2, "NEG"] == {2, 8}
    assert want[2, "MUL"] == {3, 4, 6, 7, 9, 10, 13, 15, 16, 17} and want[2, "SQR"] == {3, 5, 6, 12, 13, 15, 16, 17}
    assert want[2, "SUB"] == set(range(2, 10)) | {12, 13}


def test_raw_hooks_refuse_a_null_context_and_null_pointers():
    lib = th.load_hooks_library()
    a, out = np.zeros((1, 45), np.uint32), np.zeros((1, 18), np.uint32)
    for op in fc.ALL_OPS:
        fn = lib.msm_test_fq_raw_op if op[0] == 1 else lib.msm_test_fq2_raw_op
        assert fn(None, fc.op_word(op), mh._p32(a), mh._p32(out), 1) == mh.ERR_BAD_ARG
    assert not out.any()


def test_raw_wrappers_check_shapes_and_ops_before_the_call():
    """a row one record short would let the C hook read past the buffer: the wrapper raises before it calls (no context is touched)"""
    for call, op_of, ops in ((th.HooksContext.test_fq_raw_op, th.fq_raw_op, [o for o in fc.ALL_OPS if o[0] == 1]),
                             (th.HooksContext.test_fq2_raw_op, th.fq2_raw_op, [o for o in fc.ALL_OPS if o[0] == 2])):
        for op in ops:
            w = fc.in_words(op)
            for bad in (np.zeros((3, w - 9), np.uint32), np.zeros((3, w + 9), np.uint32), np.zeros(w, np.uint32), np.zeros((3, w - 1), np.uint32)):
                with pytest.raises(ValueError):
                    call(None, op_of(op[1], op[2]), bad)
        with pytest.raises(ValueError):
            call(None, 0xFF, np.zeros((3, 18), np.uint32))            # an unknown kind
        with pytest.raises(ValueError):
            call(None, op_of("SUB", 11), np.zeros((3, 36), np.uint32))  # a K that is not instantiated
        with pytest.raises(ValueError):
            call(None, op_of("ADD", 2), np.zeros((3, 36), np.uint32))   # a K where the function has none


# ---- the model -------------------------------------------------------------------------------------------------------------------------------
def all_launches(n_chain):
    """[(name, op, rows)]: every launch the device test makes -- the random classes of every (kind, K) at every size, each edge class, the round
    trips, a * inv(a), the composition compared with msm_test_fp_op and the sixteen rounds of the chain (fed forward by the model: the outputs are asserted equal to it, so these are the operands
    the device feeds back)"""
    rnd = random.Random(0xF9)
    out = []
    for op in fc.ALL_OPS:
        for n in SIZES:
            out.append(("random %s n=%d" % (fc.op_name(op), n), op, fc.random_launch(op, n, rnd)))
    edges = fc.edge_classes(rnd)
    for name, (op, rows) in edges.items():
        out.append((name, op, rows))
    w = fc.roundtrip_patterns(rnd)
    for a, b in (("UNPACK", "PACK"), ("FROM_STD", "TO_STD"), ("FROM_MONT256", "TO_MONT256")):
        out.append(("round trip " + a, (1, a, 0), w))
        out.append(("round trip " + b, (1, b, 0), [fc.model((1, a, 0), x) for x in w]))
    inv_rows = edges["inv"][1]
    out.append(("a * inv(a)", (1, "MUL", 0), [x + fc.model((1, "INV", 0), x) for x in inv_rows]))

    def recording(op, rows):
        out.append(("composed %s" % fc.op_name(op), op, rows))
        return [fc.model(op, r) for r in rows]

    fc.crosscheck_launches(recording, fc.crosscheck_values(rnd))
    x, y = fc.chain_start(rnd, n_chain)
    for s in range(fc.CHAIN_ROUNDS):
        x, y = fc.chain_round(recording, s, x, y)
    assert max(fc.value(r) for r in x) > 2 * P  # the chain did leave the reduced range
    return out


@pytest.fixture(scope="module")
def launches():
    return all_launches(65)  # the chain as wide as on the device: the same operands, launch for launch


def test_tables_and_builders():
    fc.check_tables()
    assert fc.value(fc.rep(1)) == fc.R261 % P and fc.rep(0) == [0] * 9 and fc.value32(fc.words8(fc.R256 - 1)) == fc.R256 - 1
    rnd = random.Random(5)
    for _ in range(50):
        ls = fc.limbs(rnd.randrange(fc.R261))
        fat = fc.fatten(ls, rnd)
        assert fc.value(fat) == fc.value(ls) and fc.model((1, "NORMALIZE", 0), fat) == ls
    # a wrong limb in a pad row, or FP2_PAD built without the - 1 of its top limb, does not pass the table check
    for k in (2, 6, 12):
        for i in range(9):
            row = list(fc.FP29_PAD[k])
            row[i] ^= 1
            with pytest.raises(AssertionError):
                fc.check_pad_row(row, k)
    for i in range(9):
        row = list(fc.FP29_PAD5_FAT3)
        row[i] -= 1
        with pytest.raises(AssertionError):
            fc.check_pad_row(row, 5, fat=3)
    for k in range(2, fc.FP2_MAX_PAD + 1):
        with pytest.raises(AssertionError):
            fc.check_pad_row(fc.make_fp2_pads(drop_minus_one=True)[k], k)
    # the contracts: 128p is inside fp_mul's and fp_sqr's (168.78p), outside fp_mul_add's (119.3p with four equal bounds)
    big = fc.limbs(128 * P - 1)
    assert fc.is_legal((1, "MUL", 0), big + big) and fc.is_legal((1, "SQR", 0), big) and not fc.is_legal((1, "MUL_ADD", 0), big * 4)
    assert 2 * (128 * P - 1) ** 2 >> 261 >= fc.R261  # even with m = 0 the top limb leaves 29 bits
    assert fc.is_legal((1, "MUL_ADD", 0), fc.limbs(fc.SQ2) * 4) and not fc.is_legal((1, "MUL_ADD", 0), fc.limbs(fc.SQ2 + 1) * 4)
    assert fc.is_legal((1, "SQR", 0), fc.limbs(fc.SQ)) and not fc.is_legal((1, "SQR", 0), fc.limbs(fc.SQ + 1))
    assert fc.is_legal((1, "MUL_ADD", 0), fc._cat(168 * P, 168 * P, 0, 0)) and not fc.is_legal((1, "MUL_ADD", 0), fc._cat(168 * P, 168 * P, 17 * P, 17 * P))
    # the legality checks refuse what the headers forbid
    L = fc.limbs
    assert not fc.is_legal((1, "ADD", 0), L(fc.TOP) + L(1)) and not fc.is_legal((1, "DBL", 0), L(1 << 260))
    assert not fc.is_legal((1, "SUB", 3), L(0) + L(2 * P)) and fc.is_legal((1, "SUB", 3), L(0) + L(2 * P - 1))
    assert not fc.is_legal((1, "SUB", 2), L(fc.R261 - 2 * P) + L(0)) and fc.is_legal((1, "SUB", 2), L(fc.R261 - 2 * P - 1) + L(0))
    assert not fc.is_legal((1, "NEG", 6), L(5 * P)) and not fc.is_legal((1, "SUB_B_2C", 0), L(0) + L(2 * P) + L(P))
    assert not fc.is_legal((1, "REDUCE_LT2P", 0), L(2 * P)) and not fc.is_legal((1, "PACK", 0), L(fc.R256)) and not fc.is_legal((1, "INV", 0), L(2 * P))
    assert not fc.is_legal((1, "IS_ZERO_LT2P", 0), L(2 * P)) and not fc.is_legal((1, "NORMALIZE", 0), [0xFFFFFFFF] * 9)
    assert not fc.is_legal((1, "MUL", 0), [1 << 29] + [0] * 8 + L(1)) and not fc.is_legal((1, "SUB", 9), L(0) + L(0))
    assert not fc.is_legal((2, "MUL", 3), L(0) * 3 + L(2 * P)) and not fc.is_legal((2, "SQR", 3), L(0) + L(2 * P))
    assert not fc.is_legal((1, "Y3", 6), L(fc.TOP) + L(fc.TOP) + L(0) + L(0) + L(0))  # r * (q + 8p - x3) outside the product's limit
    # a raw factor against a raw factor overflows a column: the scan sees it
    raw = [fc.MASK + (1 << 30)] * 8 + [0]
    with pytest.raises(AssertionError):
        fc.h_mul([(raw, raw), (raw, raw)])


def test_model_agrees_with_plain_arithmetic_on_every_class(launches):
    """check_output compares the model's integer with x * y * 2^-261 mod p (and its kin), computed without the Montgomery model and without the pad
    tables, and with the documented bound, for every element of every launch: the model itself is cross-checked here"""
    seen, elements = set(), 0
    for name, op, rows in launches:
        fc.check_all(op, rows, [fc.model(op, r) for r in rows], name)
        seen.add(op)
        elements += len(rows)
        assert len(rows) <= 600
    assert seen == set(fc.ALL_OPS) and len(seen) == 73 and elements > 15000
    # the largest 64-bit column a product scan met: the Y3 kinds with the raw factors at their largest limbs
    print("largest column: %.2f * 2^58 in %s" % (fc.COLUMN["max"] / 2 ** 58, fc.COLUMN["where"]))
    assert 27 << 58 < fc.COLUMN["max"] < 1 << 64 and fc.COLUMN["where"].startswith("fq_Y3")
    edges = fc.edge_classes(random.Random(1))
    for name in ("mul with m all ones", "mul_add with m all ones"):  # the product scan's m is the model's: all limbs 2^29 - 1
        op, rows = edges[name]
        for r in rows:
            v = [fc.value(r[i:i + 9]) for i in range(0, len(r), 9)]
            assert fc.limbs(fc.mont_m(v[0] * v[1] + (v[2] * v[3] if len(v) == 4 else 0))) == [fc.MASK] * 9
    for w in fc.roundtrip_patterns(random.Random(2)):
        assert fc.model((1, "PACK", 0), fc.model((1, "UNPACK", 0), w)) == w
        assert fc.value32(fc.model((1, "TO_STD", 0), fc.model((1, "FROM_STD", 0), w))) == fc.value32(w) % P
        assert fc.value32(fc.model((1, "TO_MONT256", 0), fc.model((1, "FROM_MONT256", 0), w))) == fc.value32(w) % P
    for v in (fc.R261 % P, 5, P - 1, P + 12345):  # a * inv(a) = rep(1)
        prod = fc.model((1, "MUL", 0), fc.limbs(v) + fc.model((1, "INV", 0), fc.limbs(v)))
        assert fc.value(prod) % P == fc.R261 % P


def test_check_output_rejects_what_it_exists_to_catch():
    rnd = random.Random(9)
    MUL, L = (1, "MUL", 0), fc.limbs
    a, b = L(rnd.randrange(84 * P)), L(rnd.randrange(84 * P))
    good = fc.model(MUL, a + b)
    fc.check_output(MUL, a + b, good)
    rejected = {"value + p": L(fc.value(good) + P), "one limb off": [good[0] ^ 1] + good[1:], "top limb off": good[:8] + [good[8] + 1]}
    carry = list(good)  # the same integer, one limb at 2^29 or more
    i = next(k for k in range(8) if carry[k + 1] > 0)
    carry[i] += 1 << 29
    carry[i + 1] -= 1
    assert fc.value(carry) == fc.value(good)
    rejected["not normalised"] = carry
    for what, bad in rejected.items():
        with pytest.raises(AssertionError):
            fc.check_output(MUL, a + b, bad, what)
    x = L(P + 5)
    for kind in ("REDUCE_LT2P", "CANONICAL"):
        for bad in (L(P + 5), L(6), L(4)):  # not reduced; reduced wrongly
            with pytest.raises(AssertionError):
                fc.check_output((1, kind, 0), x, bad)
    fc.check_output((1, "REDUCE_LT2P", 0), x, L(5))
    for kind, shift in (("UNPACK", 0), ("UNPACK_SHL5", 5)):
        w = fc.words8(rnd.getrandbits(256))
        un = fc.model((1, kind, 0), w)
        assert fc.value(un) == fc.value32(w) << shift
        for k in range(9):                                               # a bit moved to the wrong limb
            bad = list(un)
            bad[k] ^= 1 << 28
            with pytest.raises(AssertionError):
                fc.check_output((1, kind, 0), w, bad)
        if shift:                                                        # the words shifted by 4 instead of 5
            with pytest.raises(AssertionError):
                fc.check_output((1, kind, 0), w, [(fc.value32(w) << 4 >> (29 * i)) & fc.MASK for i in range(9)])
    w = fc.words8(rnd.getrandbits(256))
    un = fc.model((1, "UNPACK", 0), w)
    packed = fc.model((1, "PACK", 0), un)
    assert packed == w[:8] + [0]
    with pytest.raises(AssertionError):
        fc.check_output((1, "PACK", 0), un, packed[:8] + [1])         # word 8 must be written as 0
    for k_used in (2, 4):                                                # a + 2p - b, a + 4p - b for a + 3p - b: a wrong pad row
        with pytest.raises(AssertionError):
            fc.check_output((1, "SUB", 3), a + L(P), L(fc.value(a) + k_used * P - P))
    with pytest.raises(AssertionError):                                  # fp2_sub with the pad's top limb one too high: value + 2^232
        fc.check_output((2, "SUB", 9), a + b + L(P) + L(P), L(fc.value(a) + 8 * P + (1 << 232)) + L(fc.value(b) + 8 * P))
    sq = fc.model((1, "SQR", 0), a)
    with pytest.raises(AssertionError):                                  # a square with one cross product taken twice
        extra = fc.value(a) ** 2 + 2 * a[0] * a[1] * (1 << 29)
        fc.check_output((1, "SQR", 0), a, L(fc.closed_mont(extra)))
    fc.check_output((1, "SQR", 0), a, sq)
    with pytest.raises(AssertionError):
        fc.check_output((1, "IS_ZERO_LT2P", 0), L(P), [0] * 9)           # p is zero
    with pytest.raises(AssertionError):
        fc.check_output((1, "IS_ZERO_LT2P", 0), L(P + 1), [1] + [0] * 8)
    with pytest.raises(AssertionError):
        fc.check_all(MUL, [a + b], [good, good])
    with pytest.raises(AssertionError):                                  # an illegal operand is refused by the model, whatever the output
        fc.check_output(*fc.ILLEGAL_MUL_ADD[:1], fc.ILLEGAL_MUL_ADD[1][0], good)


# ---- the host compile of fp_bn254.hpp and fp2_bn254.hpp, every assertion live ----------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("fq_bounds_check")
    exe = d / "fq_bounds_check"
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-DFP_BOUNDS_CHECK", "-x", "hip", "--cuda-host-only",  # host code only: no device pass
                    os.path.join(ROOT, "tools", "fq_bounds_check.cpp"), "-o", str(exe)], check=True, capture_output=True, timeout=900)
    return d, exe


def write_launches(path, items):
    flat = []
    for _, op, rows in items:
        flat += fc.launch_words(op, rows)
    np.array(flat, np.uint32).tofile(path)


def test_host_run_fires_no_assertion_and_returns_the_models_limbs(driver, launches):
    d, exe = driver
    fin, fout = d / "in.bin", d / "out.bin"
    write_launches(fin, launches)
    r = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    elements = sum(len(rows) for _, _, rows in launches)
    assert r.stdout.strip().split("\n")[-1] == "%d launches, %d elements, no bound violated" % (len(launches), elements)
    got = np.fromfile(fout, np.uint32)
    at = 0
    for name, op, rows in launches:
        size = len(rows) * fc.out_words(op)
        fc.check_all(op, rows, got[at:at + size].reshape(len(rows), -1), name)  # every element of every launch
        at += size
    assert at == len(got)


def test_negative_control_mul_add_of_four_times_128p_aborts(driver):
    """four operands just below 128p: each normalised and inside the header's former "< 128p", the two products together outside
    A*B + C*D < (2^261 - p) * 2^261.  The host program, in a child process of its own, must die on the new assertion in fp_mul_add: the assertions
    are compiled in, and the former contract was false.  A CPU program only: nothing illegal is ever handed to the device hook"""
    d, exe = driver
    fin, fout = d / "illegal.bin", d / "illegal_out.bin"
    write_launches(fin, [("illegal",) + fc.ILLEGAL_MUL_ADD])
    r = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "fp_mul_add: result not normalised" in r.stderr, (r.returncode, r.stdout, r.stderr)
    assert "no bound violated" not in r.stdout and not fout.exists()
    # the classes just below the limit beside it pass
    edges = fc.edge_classes(random.Random(1))
    write_launches(fin, [(name,) + edges[name] for name in ("mul_add just below its limit", "mul top of the domain",
                                                            "sqr fullest middle columns and the largest square")])
    r = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "no bound violated" in r.stdout, r.stderr
    # fp_reduce_lt2p silently returns a non-canonical value for an input of 2p or more: the bounds-check build does not
    for bad in (2 * P, 3 * P + 5):
        write_launches(fin, [("2p", (1, "REDUCE_LT2P", 0), [fc.limbs(bad)])])
        r = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True, timeout=600)
        assert r.returncode != 0 and "fp_reduce_lt2p: input was >= 2p" in r.stderr, (r.returncode, r.stderr)
