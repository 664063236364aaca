"""Limb-range proof-by-assertion for the lazily reduced G2 group law (CPU test, no GPU), and the CPU side of its device hook.

fp2_bn254.hpp / ec_g2_bn254.hpp are __host__ __device__; tools/g2_bounds_check.cpp compiles them for the host with -DFP_BOUNDS_CHECK, which
turns every range assumption (pad >= subtrahend limb, no 32-bit limb overflow, no 64-bit column overflow, value < 2^261) into an abort.  It
drives every fp2_mul<K> / fp2_sqr<K> / fp2_sub<K> / fp2_neg<K> the G2 code instantiates, xyzz2_madd / xyzz2_add / xyzz2_dbl on operands at the
very top of their documented ranges (X < 12p, Y < 8p, ZZ, ZZZ < 4.2p), the special cases and long mixed chains, checks that every output is back
inside those ranges, and compares residues with the independent 4 x 64-bit host arithmetic (host_g2.hpp).
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mopro_msm_hip as mh
from mopro_msm_hip import testhooks as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_g2_limb_bounds_hold(tmp_path):
    exe = tmp_path / "g2_bounds_check"
    cmd = ["hipcc", "-O2", "-std=c++17", "-DFP_BOUNDS_CHECK", "-x", "hip", "--cuda-host-only",  # host code only: no device pass
           os.path.join(ROOT, "tools", "g2_bounds_check.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.strip().split("\n")
    assert "no bound violated" in lines[-1]
    # the margin to the documented bounds is on record in the output, and the driver did compute on something
    m = re.search(r"X ([0-9.]+) \(< 12\), Y ([0-9.]+) \(< 8\), ZZ ([0-9.]+) \(< 4.2\), ZZZ ([0-9.]+) \(< 4.2\)", r.stdout)
    assert m, r.stdout[-2000:]
    x, y, zz, zzz = (float(v) for v in m.groups())
    assert 1 < x < 12 and 1 < y < 8 and 1 < zz < 4.2 and 1 < zzz < 4.2


def test_g2_op_hook_lives_in_the_hooks_build_only():
    assert "msm_test_g2_op" in th.HOOK_SYMBOLS
    assert hasattr(th.load_hooks_library(), "msm_test_g2_op") and not hasattr(mh.load_library(), "msm_test_g2_op")
    hdr = open(os.path.join(ROOT, "include", "msm_hip_testhooks.h")).read()
    for name, val in (("MSM_OP_G2_MADD", th.OP_G2_MADD), ("MSM_OP_G2_ADD", th.OP_G2_ADD), ("MSM_OP_G2_DBL", th.OP_G2_DBL)):
        assert re.search(r"#define %s %du\b" % (name, val), hdr), name
    assert "msm_test_g2_op" not in open(os.path.join(ROOT, "include", "msm_hip.h")).read()


def test_g2_op_hook_refuses_a_null_context():
    lib = th.load_hooks_library()
    a, b, out = np.zeros((1, 72), np.uint32), np.zeros((1, 72), np.uint32), np.zeros((1, 72), np.uint32)
    for op in (th.OP_G2_MADD, th.OP_G2_ADD, th.OP_G2_DBL):
        assert lib.msm_test_g2_op(None, op, mh._p32(a), mh._p32(b), mh._p32(out), 1) == mh.ERR_BAD_ARG
    assert not out.any()


def test_g2_op_wrapper_checks_shapes_before_the_call():
    """a missing or shorter b would let the C hook read past the buffer: the wrapper raises before it calls (no context is touched)"""
    call = th.HooksContext.test_g2_op
    a = np.zeros((3, 72), np.uint32)
    for op, b in ((th.OP_G2_MADD, None), (th.OP_G2_ADD, None), (th.OP_G2_MADD, np.zeros((2, 36), np.uint32)),
                  (th.OP_G2_ADD, np.zeros((2, 72), np.uint32)), (3, a)):
        with pytest.raises(ValueError):
            call(None, op, a, b)
    with pytest.raises(ValueError):
        call(None, th.OP_G2_DBL, np.zeros(71, np.uint32))  # not a whole record
