"""The BN254 base field Fq and Fq2 on the device, one function at a time (-m gpu), on RAW limb records: every function of csrc/fp_bn254.hpp and
csrc/fp2_bn254.hpp, at every pad multiple K the sources instantiate, through msm_test_fq_raw_op / msm_test_fq2_raw_op, which hand the kernel the
words the test wrote and return the limbs it stored.  msm_test_fp_op (tests/test_gpu_1_parity.py) only ever shows six of these functions fresh
fp_mul outputs below 1.01p and hides the representative of the result behind fp_to_mont256; the group-law tests (tests/test_gpu_15, _20) reach the
rest with the operands the formulas make.  Here the test chooses the operand -- products at the top of A*B (+ C*D) < (2^261 - p) * 2^261, raw
factors at their largest limbs (the fullest 64-bit columns), carries and borrows through all nine limbs, subtrahends one below (K-1)p, p itself and
its neighbours -- and checks EVERY element of every launch with tools/fq_ops_cases.check_output: the limbs equal the integer model's limb for limb,
every limb <= 2^29 - 1, the value inside the bound the header documents, and congruent modulo p to the plain-arithmetic result.  Integer work: no
tolerance anywhere.  tools/fq_bounds_check.cpp (tests/test_fq_ops_cpu.py) runs the same launches through the host compile with every limb
assumption asserted: that is the check that these inputs are legal.  Nothing illegal is handed to the device."""
import os
import random
import sys

import numpy as np
import pytest

import mopro_msm_hip as mh
from mopro_msm_hip import testhooks as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fq_ops_cases as fc  # noqa: E402

pytestmark = pytest.mark.gpu
P = fc.P
SIZES = (1, 63, 64, 65)
EDGE_NAMES = sorted(fc.edge_classes(random.Random(0)))  # the names do not depend on the seed


def arr(rows):
    return np.array(rows, np.uint32)


# ---- shared operands, made once --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    c = th.HooksContext()
    yield c
    c.close()


@pytest.fixture(scope="module")
def data():
    rnd = random.Random(0xF9)
    d = {"random": {}}
    for op in fc.ALL_OPS:
        for n in SIZES:
            d["random"][op, n] = fc.random_launch(op, n, rnd)
    d["edges"] = fc.edge_classes(rnd)
    assert sorted(d["edges"]) == EDGE_NAMES and max(len(v[1]) for v in d["edges"].values()) <= 600
    d["patterns"] = fc.roundtrip_patterns(rnd)
    d["crosscheck"] = fc.crosscheck_values(rnd)  # (drawn in the order of tests/test_fq_ops_cpu.py's all_launches: the host ran the same operands)
    d["chain"] = fc.chain_start(rnd, 65)
    return d


def run(ctx, op, rows):
    call = ctx.test_fq_raw_op if op[0] == 1 else ctx.test_fq2_raw_op
    return call(fc.op_word(op), arr(rows))


def run_checked(ctx, op, rows, what):
    out = run(ctx, op, rows)
    fc.check_all(op, rows, out, what)  # every element
    return [[int(w) for w in r] for r in out]


# ---- 1. every kind and K on the random classes: one lane, a wavefront less one, a full wavefront, a wavefront and a partial workgroup ------------
@pytest.mark.parametrize("op", fc.ALL_OPS, ids=[fc.op_name(op) for op in fc.ALL_OPS])
def test_random_classes(ctx, data, op):
    for n in SIZES:
        rows = data["random"][op, n]
        assert len(rows) == n
        run_checked(ctx, op, rows, "random %s n=%d" % (fc.op_name(op), n))


# ---- 2. each edge class in a launch of its own ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EDGE_NAMES)
def test_edge_class(ctx, data, name):
    op, rows = data["edges"][name]
    run_checked(ctx, op, rows, name)


def test_round_trips(ctx, data):
    w = data["patterns"]
    un = run_checked(ctx, (1, "UNPACK", 0), w, "unpack")
    assert run_checked(ctx, (1, "PACK", 0), un, "pack(unpack)") == [x[:8] + [0] for x in w]
    for a, b in (("FROM_STD", "TO_STD"), ("FROM_MONT256", "TO_MONT256")):
        inner = run_checked(ctx, (1, a, 0), w, a)
        back = run_checked(ctx, (1, b, 0), inner, "%s(%s)" % (b, a))
        assert [fc.value32(x) for x in back] == [fc.value32(x) % P for x in w]


def test_inverse_times_itself_is_one(ctx, data):
    op, rows = data["edges"]["inv"]
    inv = run_checked(ctx, op, rows, "inv")
    prod = run_checked(ctx, (1, "MUL", 0), [a + i for a, i in zip(rows, inv)], "a * inv(a)")
    for a, p in zip(rows, prod):
        assert fc.value(p) % P == (fc.R261 % P if fc.value(a) % P else 0)
    assert not any(inv[0]) and not any(rows[0])  # 0 gives 0, limb for limb


# ---- 3. the Y3 of the mixed addition as a chain of sixteen rounds, the device's own outputs fed back -------------------------------------------
def test_chain_of_sixteen_rounds(ctx, data):
    x, y = data["chain"]
    go = fc.checked(lambda op, rows: run(ctx, op, rows))
    for s in range(fc.CHAIN_ROUNDS):
        x, y = fc.chain_round(go, s, x, y)
    assert max(fc.value(r) for r in x) > 2 * P  # the values did leave the reduced range


# ---- 4. the existing path: msm_test_fp_op on canonical words ---------------------------------------------------------------------------------
def test_raw_hook_agrees_with_msm_test_fp_op(ctx, data):
    """ops 2, 3, 4 of msm_test_fp_op (fp_to_mont256(fp_mul(fp_from_mont256 a, fp_from_mont256 b)), fp_to_mont256(fp_from_std a),
    fp_to_std(fp_from_mont256 a)) on canonical words: the same words through the raw hook, one function per launch"""
    raw, a, b = fc.crosscheck_launches(fc.checked(lambda op, rows: run(ctx, op, rows)), data["crosscheck"])
    a8, b8 = arr(a)[:, :8].copy(), arr(b)[:, :8].copy()
    for op, got in raw.items():
        public = ctx.test_fp_op(op, a8, b8 if op == 2 else None)
        assert (arr(got)[:, :8] == public).all(), op


# ---- 5. the hooks' own argument checks -------------------------------------------------------------------------------------------------------
def test_hooks_refuse_malformed_input(ctx, data):
    lib, h = ctx._lib, ctx._h
    out = np.zeros((2, 18), np.uint32)
    for field, fn in ((1, lib.msm_test_fq_raw_op), (2, lib.msm_test_fq2_raw_op)):
        ops = [op for op in fc.ALL_OPS if op[0] == field]
        for op in ops:
            rows = arr(data["random"][op, 63][:2])
            word = fc.op_word(op)
            call = lambda w, rows_, n: fn(h, w, mh._p32(rows_), mh._p32(out), n)
            assert call(word, rows, 0) == mh.ERR_EMPTY
            assert fn(h, word, None, mh._p32(out), 2) == mh.ERR_BAD_ARG and fn(h, word, mh._p32(rows), None, 2) == mh.ERR_BAD_ARG
            if field == 1 and op[1] in ("NORMALIZE",) + fc.WORDS_IN:
                continue  # any 32-bit words
            for at in (0, 8, rows.shape[1] - 1, rows.shape[1] + 8):  # a limb of 2^29 or more is refused before anything runs
                bad = rows.copy()
                bad.reshape(-1)[at] = 1 << 29
                assert call(word, bad, 2) == mh.ERR_BAD_ARG, fc.op_name(op)
        kinds = fc.FQ_KINDS if field == 1 else fc.FQ2_KINDS
        ks = fc.FQ_K if field == 1 else fc.FQ2_K
        rows = np.zeros((2, 45), np.uint32)
        for word in (len(kinds), 0xFF, 0xFFFFFFFF, 1 << 8, kinds.index("SUB"), kinds.index("SUB") | 11 << 8, kinds.index("SUB") | 1 << 8,
                     kinds.index("ADD") | 2 << 8, kinds.index("NEG") | 5 << 8):
            assert (word & 0xFF) >= len(kinds) or (word >> 8) not in ks.get(kinds[word & 0xFF], (0,))
            assert fn(h, word, mh._p32(rows), mh._p32(out), 2) == mh.ERR_BAD_ARG, word
    assert not out.any()  # nothing was written by any refused call
    bad = arr(data["random"][(1, "MUL", 0), 63][:2])
    bad[1, 17] = 1 << 29
    with pytest.raises(mh.MsmError) as e:
        ctx.test_fq_raw_op(fc.op_word((1, "MUL", 0)), bad)
    assert e.value.code == mh.ERR_BAD_ARG
    for op in ((1, "MUL_ADD", 0), (2, "MUL", 17)):
        run_checked(ctx, op, data["random"][op, 63], "the context still works")
