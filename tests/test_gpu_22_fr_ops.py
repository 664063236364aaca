"""The BN254 scalar field Fr on the device, one function at a time (-m gpu), on RAW limb records: fr_mul, fr_add, fr_sub<2 / 3 / 7 / 8>,
fr_normalize, fr_reduce_lt2r, fr_canonical, fr_unpack, fr_pack, fr_from_std, fr_to_std, fr_pow_u32 and fr_inv of csrc/fr_bn254.hpp through
msm_test_fr_raw_op, which hands the kernel the nine words the test wrote and returns the nine limbs it stored.  The transforms, the setup scalars
and the R1CS rows (tests/test_gpu_9, _10, _13) only ever show these functions the representatives a whole algorithm makes of 8-word inputs, and
hide the representative of the result behind fr_reduce_lt2r and fr_pack; here the test chooses the operand -- values next to 2^261, limb patterns
that ripple a carry or a borrow through all nine limbs, subtrahends one below the pad's limit -- and checks EVERY element of every launch with
tools/fr_ops_cases.check_output: the limbs equal the integer model's limb for limb, every limb <= 2^29 - 1, the value inside the bound the header
documents, and congruent modulo r to the plain-arithmetic result.  Integer work: no tolerance anywhere.
tools/fr_bounds_check.cpp (tests/test_fr_ops_cpu.py) runs the same operand classes through the host compile with every limb assumption asserted:
that is the check that these inputs are legal.  Nothing illegal is handed to the device."""
import os
import random
import sys

import numpy as np
import pytest

import mopro_msm_hip as mh
from mopro_msm_hip import testhooks as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fr_ops_cases as fc  # noqa: E402

pytestmark = pytest.mark.gpu
R = fc.R
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
    rnd = random.Random(0xF2)
    d = {"rnd": rnd, "random": {}}
    for op in range(len(fc.OPS)):
        for n in SIZES:
            d["random"][op, n] = fc.random_launch(op, n, rnd)
    d["edges"] = fc.edge_classes(rnd)
    assert sorted(d["edges"]) == EDGE_NAMES and {v[0] for v in d["edges"].values()} == set(range(len(fc.OPS)))
    assert max(len(v[1]) for v in d["edges"].values()) <= 600
    d["patterns"] = fc.roundtrip_patterns(rnd)
    d["chain"] = fc.chain_start(rnd, 65)
    return d


def run(ctx, op, a, b=None):
    return ctx.test_fr_raw_op(op, arr(a), arr(b) if b is not None else None)


def run_checked(ctx, op, a, b, what):
    out = run(ctx, op, a, b)
    fc.check_all(op, a, b, out, what)  # every element
    return out


# ---- 1. every operation on the random classes: one lane, a full wavefront less one, a full wavefront, a wavefront and a partial workgroup ----
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("op", range(len(fc.OPS)), ids=fc.OPS)
def test_random_classes(ctx, data, op, n):
    a, b = data["random"][op, n]
    assert len(a) == n
    run_checked(ctx, op, a, b, "random %s n=%d" % (fc.OPS[op], n))


# ---- 2. each edge class in a launch of its own ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EDGE_NAMES)
def test_edge_class(ctx, data, name):
    op, a, b = data["edges"][name]
    run_checked(ctx, op, a, b, name)


def test_round_trips(ctx, data):
    w = data["patterns"]
    un = run_checked(ctx, fc.UNPACK, w, None, "unpack")
    assert (run_checked(ctx, fc.PACK, un, None, "pack(unpack)") == arr(w)).all()
    rp = run_checked(ctx, fc.FROM_STD, w, None, "from_std")
    back = run_checked(ctx, fc.TO_STD, rp, None, "to_std(from_std)")
    assert [fc.value32(x) for x in back] == [fc.value32(x) % R for x in w]


def test_inverse_times_itself_is_one(ctx, data):
    op, a, _ = data["edges"]["inv"]
    inv = run_checked(ctx, fc.INV, a, None, "inv")
    prod = run_checked(ctx, fc.MUL, a, inv, "a * inv(a)")
    for x, p in zip(a, prod):
        assert fc.value(p) % R == (fc.R261 % R if fc.value(x) % R else 0)
    assert not inv[0].any() and not any(a[0])  # 0 gives 0, limb for limb


# ---- 3. the butterfly of ntt_bn254.hpp, twelve levels, the device's own outputs fed back -------------------------------------------------------
def test_butterfly_chain_of_twelve_levels(ctx, data):
    u, v, tw = data["chain"]
    for s in range(fc.CHAIN_LEVELS):
        u, v = fc.chain_level(lambda op, a, b: run(ctx, op, a, b), s, u, v, tw[s])
    assert max(fc.value(x) for x in list(u) + list(v)) > 2 * R  # the rows did leave the reduced range


# ---- 4. FROM_STD / TO_STD against the public path ------------------------------------------------------------------------------------------
def test_from_std_to_std_agree_with_mul_sub_scale(ctx, data):
    """fr_mul_sub_scale_device(a, b = 1, no c) is to_std(from_std(a) * from_std(1)): the same words through the product's own kernel"""
    import torch
    w = arr(data["patterns"])[:, :8].copy()
    n = len(w)
    ones = np.zeros((n, 8), np.uint32)
    ones[:, 0] = 1
    da, db = torch.from_numpy(w.view(np.int32)).cuda(), torch.from_numpy(ones.view(np.int32)).cuda()
    dout = torch.zeros_like(da)
    ctx.fr_mul_sub_scale_device(da.data_ptr(), db.data_ptr(), None, dout.data_ptr(), n)
    torch.cuda.synchronize()
    public = dout.cpu().numpy().view(np.uint32)
    rp = run_checked(ctx, fc.FROM_STD, data["patterns"], None, "from_std")
    back = run_checked(ctx, fc.TO_STD, rp, None, "to_std")
    assert (back[:, :8] == public).all() and not back[:, 8].any()
    assert [fc.value32(x) for x in public] == [fc.value32(x) % R for x in w]


# ---- 5. the hook's own argument checks -------------------------------------------------------------------------------------------------------
def test_hook_refuses_malformed_input(ctx, data):
    lib, h = ctx._lib, ctx._h
    a, b = arr(data["random"][fc.MUL, 63][0][:2]), arr(data["random"][fc.MUL, 63][1][:2])
    out = np.zeros_like(a)
    call = lambda op, a_, b_, n: lib.msm_test_fr_raw_op(h, op, mh._p32(a_), mh._p32(b_), mh._p32(out), n)
    assert call(fc.MUL, a, b, 0) == mh.ERR_EMPTY
    assert all(call(op, a, None, 2) == mh.ERR_BAD_ARG for op in fc.NEEDS_B)
    assert call(len(fc.OPS), a, b, 2) == mh.ERR_BAD_ARG and call(0xFFFFFFFF, a, b, 2) == mh.ERR_BAD_ARG
    assert lib.msm_test_fr_raw_op(h, fc.MUL, None, mh._p32(b), mh._p32(out), 2) == mh.ERR_BAD_ARG
    assert lib.msm_test_fr_raw_op(h, fc.MUL, mh._p32(a), mh._p32(b), None, 2) == mh.ERR_BAD_ARG
    for word in (0, 8, 9 + 8):  # a limb of 2^29 or more where the function needs a normalised operand is refused before anything runs
        bad = a.copy()
        bad.reshape(-1)[word] = 1 << 29
        for op in range(len(fc.OPS)):
            if op not in (fc.NORMALIZE, fc.UNPACK, fc.FROM_STD):
                assert call(op, bad, b, 2) == mh.ERR_BAD_ARG, fc.OPS[op]
            if op in fc.NEEDS_B and op != fc.POW_U32:
                assert call(op, a, bad, 2) == mh.ERR_BAD_ARG, fc.OPS[op]
    assert not out.any()  # nothing was written by any refused call
    with pytest.raises(mh.MsmError) as e:
        ctx.test_fr_raw_op(fc.MUL, bad, b)
    assert e.value.code == mh.ERR_BAD_ARG
    fc.check_all(fc.MUL, a, b, ctx.test_fr_raw_op(fc.MUL, a, b), "the context still works")
