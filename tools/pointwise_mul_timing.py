#!/usr/bin/env python3
"""The G1 element-wise multiplication on one GPU, the whole sweep in one process (run it under a time limit when the GPU is shared,
tools/README.md):

  per size 2^16, 2^18, 2^20, 2^22 (--log2 16,18,20,22): msm_bn254_g1_pointwise_mul_device (a scalar per point) and msm_bn254_g1_scale_device (one
      scalar), median and minimum of --steps calls after --warmup, by events on the call's stream; beside them, in the same process:
      msm_bn254_g1_fixed_base_mul_device on the same scalars (what a table buys when the base is shared), msm_bn254_fr_batch_inverse_device (the
      live calibration of the field-multiplication rate: 4 + 381 / inv_group multiplications per element by count), msm_bn254_g1_device on the
      points with the accumulate kernel's shader clock (a slow box shows there), and the hooks library's generate_device if it is built.

  python tools/pointwise_mul_timing.py [--steps 20] [--warmup 3] [--out profiles/pointwise_mul_timing_mi355x.txt]

The bases are k_i * G made by the fixed-base call; the first and last products are checked against the oracle.  Every result line is printed
and, with --out, appended."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "gpu-acceleration_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import mopro_msm_hip as mh  # noqa: E402
import pointwise_mul_cases as pm  # noqa: E402
from fixed_base_timing import event_ms, med_min, wall_ms  # noqa: E402

orc = pm.orc
# field multiplications per point, by count (pointwise_mul_bn254.hpp): 126 doublings of 8, the additions of 9 a wavefront executes (all 126 when
# every lane has its own scalar, the 3/4 its bits select with one scalar), and 19 around the ladder (point 2, beta x 1, S 4, the two shared
# inversions 3 each, output 6); the two field inversions of a workgroup add 2 * 335 / inv_group
MULS_DBL, MULS_MADD, MULS_REST, MULS_FP_INV, MULS_FR_INV = 8, 9, 19, 335, 381
LADDER = 126


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", default="16,18,20,22")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from mopro_msm_hip import testhooks
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(device=dev)
    s = st.cuda_stream
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    plan, G_INV = mh.pointwise_mul_plan(), mh.fr_vector_plan()["inv_group"]
    say("plan: %s" % plan)
    G = plan["inv_group"]
    muls = {"pointwise": LADDER * (MULS_DBL + MULS_MADD) + MULS_REST + 2 * MULS_FP_INV / G,
            "scale": LADDER * (MULS_DBL + 0.75 * MULS_MADD) + MULS_REST + 2 * MULS_FP_INV / G, "inverse": 4 + MULS_FR_INV / G_INV}
    sizes = [int(v) for v in a.log2.split(",") if v]
    nmax = 1 << max(sizes)
    rng = np.random.default_rng(0x9017)
    h_b = rng.integers(0, 1 << 32, size=(nmax, 8), dtype=np.uint64).astype(np.uint32)  # logarithms of the bases (read modulo r)
    h_k = rng.integers(0, 1 << 32, size=(nmax, 8), dtype=np.uint64).astype(np.uint32)  # the scalars
    one = pm.patterns(0x9018, 1)[0]
    d_b, d_k = torch.from_numpy(h_b.view(np.int32)).to(dev), torch.from_numpy(h_k.view(np.int32)).to(dev)
    d_bases = torch.zeros((nmax, 16), dtype=torch.int32, device=dev)
    d_binf = torch.zeros(nmax, dtype=torch.uint8, device=dev)
    d_xy = torch.zeros((nmax, 16), dtype=torch.int32, device=dev)
    d_inf = torch.zeros(nmax, dtype=torch.uint8, device=dev)
    d_tmp = torch.zeros((nmax, 8), dtype=torch.int32, device=dev)
    d_s = torch.from_numpy(orc.gen_scalars(0x9019, nmax).view(np.int32)).to(dev)  # canonical scalars: what the MSM beside the calls takes
    gen = np.concatenate([pm.words(1), pm.words(2)])
    torch.cuda.synchronize()

    def check(what, n, scalar_of):
        torch.cuda.synchronize()
        at = [0, 1, 2, n - 3, n - 2, n - 1]
        got = (d_xy[at].cpu().numpy().view(np.uint32), d_inf[at].cpu().numpy())
        want = pm.expected([scalar_of(i) for i in at], [orc.words_to_int(h_b[i]) for i in at])
        if not ((got[0] == want[0]).all() and (got[1] == want[1]).all()):
            raise SystemExit("WRONG RESULT at %s" % (what,))

    with mh.MsmContext(device=0) as ctx:
        ctx.fixed_base_mul_device(gen, d_b.data_ptr(), nmax, d_bases.data_ptr(), d_binf.data_ptr(), stream=s)  # P_i = b_i * G
        st.synchronize()
        for lg in sizes:
            n = 1 << lg
            ev = {}
            ev["pointwise"] = event_ms(torch, st, lambda: ctx.pointwise_mul_device(d_bases.data_ptr(), d_k.data_ptr(), n, d_xy.data_ptr(), d_inf.data_ptr(),
                                                                                  d_binf.data_ptr(), stream=s), a.steps, a.warmup)
            check(("pointwise", lg), n, lambda i: orc.words_to_int(h_k[i]))
            ev["scale"] = event_ms(torch, st, lambda: ctx.scale_device(d_bases.data_ptr(), one, n, d_xy.data_ptr(), d_inf.data_ptr(), d_binf.data_ptr(),
                                                                      stream=s), a.steps, a.warmup)
            check(("scale", lg), n, lambda i: one)
            ev["inverse"] = event_ms(torch, st, lambda: ctx.fr_batch_inverse_device(d_k.data_ptr(), d_tmp.data_ptr(), n, stream=s), a.steps, a.warmup)
            fixed = event_ms(torch, st, lambda: ctx.fixed_base_mul_device(gen, d_k.data_ptr(), n, d_xy.data_ptr(), d_inf.data_ptr(), stream=s), a.steps, a.warmup)
            for _ in range(a.warmup):
                ctx.msm_device(d_bases.data_ptr(), d_s.data_ptr(), n, d_binf.data_ptr())
            ctx.reset_kernel_stats()
            ctx.set_kernel_timing(1)
            msm = wall_ms(torch, lambda: ctx.msm_device(d_bases.data_ptr(), d_s.data_ptr(), n, d_binf.data_ptr()), a.steps, 0)
            ctx.set_kernel_timing(0)
            sclk = ctx.clock_stats()["sclk_ghz"]
            rate = {name: muls[name] * n / (statistics.median(ms) * 1e6) for name, ms in ev.items()}  # G multiplications / s
            med = {name: statistics.median(ms) for name, ms in ev.items()}
            say(f"2^{lg}: pointwise_mul_device {med_min(ev['pointwise'])} by events, {muls['pointwise']:.0f} multiplications per point by count = "
                f"{rate['pointwise']:.1f} G/s, {med['pointwise'] * 1e6 / n:.1f} ns per point")
            say(f"2^{lg}: scale_device {med_min(ev['scale'])} by events, {muls['scale']:.0f} multiplications per point by count = {rate['scale']:.1f} G/s; "
                f"per-element / one scalar = {med['pointwise'] / med['scale']:.3f} x (by count {muls['pointwise'] / muls['scale']:.3f} x)")
            say(f"2^{lg}: fr_batch_inverse_device {med_min(ev['inverse'])} by events, {muls['inverse']:.2f} multiplications per element by count = "
                f"{rate['inverse']:.1f} G/s")
            say(f"2^{lg}: fixed_base_mul_device {med_min(fixed)} by events: pointwise / fixed base = {med['pointwise'] / statistics.median(fixed):.1f} x; "
                f"G1 MSM on these points {med_min(msm)} by the host clock at sclk {sclk:.3f} GHz")
        if os.path.exists(testhooks.HOOKS_LIB_PATH):
            n = 1 << max(s_ for s_ in sizes if s_ <= 20) if any(s_ <= 20 for s_ in sizes) else 1 << min(sizes)
            with testhooks.HooksContext(device=0) as h:
                hk = wall_ms(torch, lambda: h.generate_device(0xB2540031, 0, n, d_xy.data_ptr(), None), max(3, a.steps // 4), 1)
            say(f"2^{n.bit_length() - 1}: hooks generate_device (254 one-bit windows of the generator, one inversion per point) {med_min(hk)} by the host clock")
        else:
            say("the hooks library is not built: no generate_device beside it")
    say("device: %s" % torch.cuda.get_device_name(0))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
