#!/usr/bin/env python3
"""The G2 element-wise multiplication on one GPU, the whole sweep in one process (run it under a time limit when the GPU is shared,
tools/README.md):

  per size 2^16, 2^18, 2^20 (--log2 16,18,20): msm_bn254_g2_pointwise_mul_device (a scalar per point) and msm_bn254_g2_scale_device (one scalar),
      median and minimum of --steps calls after --warmup, by events on the call's stream; beside them, in the same process: the G1 per-element
      and one-scalar calls on as many points (the yardstick: their time times the ratio of field work), msm_bn254_g2_fixed_base_mul_device on the
      same scalars (what a table buys when the base is shared), and msm_bn254_g1_device with the accumulate kernel's shader clock (a slow box
      shows there).

  python tools/g2_pointwise_mul_timing.py [--steps 20] [--warmup 3] [--out profiles/g2_pointwise_mul_timing_mi355x.txt]

The bases are b_i * H resp. b_i * G made by the fixed-base calls; the first and last records of every output array are checked word for word
against the Python models.  Every result line is printed and, with --out, appended."""
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
import g2_pointwise_mul_cases as pm2  # noqa: E402
from fixed_base_timing import event_ms, med_min, wall_ms  # noqa: E402

pm, fb2 = pm2.pm, pm2.fb2
orc = pm.orc
# by count (g2_pointwise_mul_bn254.hpp, pointwise_mul_bn254.hpp).  Units: field multiplications, an fp2_mul or fp2_sqr being two.  Limb products:
# fp_mul 162, fp2_sqr 324, fp2_mul 486; xyzz2_dbl = 3 fp2_sqr + 6 fp2_mul, xyzz2_madd = 2 fp2_sqr + 8 fp2_mul; G1: xyzz_dbl 8, xyzz_madd 9 fp_mul
LADDER = 126
G2_UNITS = {"pointwise": LADDER * (18 + 20) + 42, "scale": LADDER * (18 + 0.75 * 20) + 42}
G1_UNITS = {"pointwise": LADDER * (8 + 9) + 19, "scale": LADDER * (8 + 0.75 * 9) + 19}
G2_LIMB = {"pointwise": LADDER * (3888 + 4536), "scale": LADDER * (3888 + 0.75 * 4536)}
G1_LIMB = {"pointwise": LADDER * (8 + 9) * 162, "scale": LADDER * (8 + 0.75 * 9) * 162}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", default="16,18,20")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(device=dev)
    s = st.cuda_stream
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say("plan: %s" % mh.g2_pointwise_mul_plan())
    say("by count, G2 / G1: per-element %.3f x in units (%d / %d), %.3f x in limb products; one scalar %.3f x in units, %.3f x in limb products"
        % (G2_UNITS["pointwise"] / G1_UNITS["pointwise"], G2_UNITS["pointwise"], G1_UNITS["pointwise"], G2_LIMB["pointwise"] / G1_LIMB["pointwise"],
           G2_UNITS["scale"] / G1_UNITS["scale"], G2_LIMB["scale"] / G1_LIMB["scale"]))
    sizes = [int(v) for v in a.log2.split(",") if v]
    nmax = 1 << max(sizes)
    rng = np.random.default_rng(0x9027)
    h_b = rng.integers(0, 1 << 32, size=(nmax, 8), dtype=np.uint64).astype(np.uint32)  # logarithms of the bases (read modulo r)
    h_k = rng.integers(0, 1 << 32, size=(nmax, 8), dtype=np.uint64).astype(np.uint32)  # the scalars
    one = pm.patterns(0x9028, 1)[0]
    d_b, d_k = torch.from_numpy(h_b.view(np.int32)).to(dev), torch.from_numpy(h_k.view(np.int32)).to(dev)
    d_q, d_xy2 = (torch.zeros((nmax, 32), dtype=torch.int32, device=dev) for _ in range(2))
    d_p, d_xy1 = (torch.zeros((nmax, 16), dtype=torch.int32, device=dev) for _ in range(2))
    d_qinf, d_pinf, d_inf2, d_inf1 = (torch.zeros(nmax, dtype=torch.uint8, device=dev) for _ in range(4))
    d_s = torch.from_numpy(orc.gen_scalars(0x9029, nmax).view(np.int32)).to(dev)  # canonical scalars: what the MSM beside the calls takes
    gen1, gen2 = np.concatenate([pm.words(1), pm.words(2)]), fb2.base_words(pm2.GEN)
    torch.cuda.synchronize()

    def check(what, n, scalar_of, g2_side=True, base_of=lambda i: orc.words_to_int(h_b[i])):
        torch.cuda.synchronize()
        at = [0, 1, 2, n - 3, n - 2, n - 1]
        xy, inf, model = (d_xy2, d_inf2, pm2) if g2_side else (d_xy1, d_inf1, pm)
        got = (xy[at].cpu().numpy().view(np.uint32), inf[at].cpu().numpy())
        want = model.expected([scalar_of(i) for i in at], [base_of(i) for i in at])
        if not ((got[0] == want[0]).all() and (got[1] == want[1]).all()):
            raise SystemExit("WRONG RESULT at %s" % (what,))

    k_of = lambda i: orc.words_to_int(h_k[i])  # noqa: E731
    with mh.MsmContext(device=0) as ctx:
        ctx.fixed_base_g2_mul_device(gen2, d_b.data_ptr(), nmax, d_q.data_ptr(), d_qinf.data_ptr(), stream=s)  # Q_i = b_i * H
        ctx.fixed_base_mul_device(gen1, d_b.data_ptr(), nmax, d_p.data_ptr(), d_pinf.data_ptr(), stream=s)      # P_i = b_i * G
        st.synchronize()
        for lg in sizes:
            n = 1 << lg
            ev = {}
            ev["g2 pointwise"] = event_ms(torch, st, lambda: ctx.g2_pointwise_mul_device(d_q.data_ptr(), d_k.data_ptr(), n, d_xy2.data_ptr(), d_inf2.data_ptr(),
                                                                                        d_qinf.data_ptr(), stream=s), a.steps, a.warmup)
            check(("g2 pointwise", lg), n, k_of)
            ev["g2 scale"] = event_ms(torch, st, lambda: ctx.g2_scale_device(d_q.data_ptr(), one, n, d_xy2.data_ptr(), d_inf2.data_ptr(), d_qinf.data_ptr(),
                                                                            stream=s), a.steps, a.warmup)
            check(("g2 scale", lg), n, lambda i: one)
            ev["g1 pointwise"] = event_ms(torch, st, lambda: ctx.pointwise_mul_device(d_p.data_ptr(), d_k.data_ptr(), n, d_xy1.data_ptr(), d_inf1.data_ptr(),
                                                                                     d_pinf.data_ptr(), stream=s), a.steps, a.warmup)
            check(("g1 pointwise", lg), n, k_of, False)
            ev["g1 scale"] = event_ms(torch, st, lambda: ctx.scale_device(d_p.data_ptr(), one, n, d_xy1.data_ptr(), d_inf1.data_ptr(), d_pinf.data_ptr(),
                                                                         stream=s), a.steps, a.warmup)
            check(("g1 scale", lg), n, lambda i: one, False)
            ev["g2 fixed"] = event_ms(torch, st, lambda: ctx.fixed_base_g2_mul_device(gen2, d_k.data_ptr(), n, d_xy2.data_ptr(), d_inf2.data_ptr(), stream=s),
                                      a.steps, a.warmup)
            check(("g2 fixed base", lg), n, k_of, base_of=lambda i: 1)
            for _ in range(a.warmup):
                ctx.msm_device(d_p.data_ptr(), d_s.data_ptr(), n, d_pinf.data_ptr())
            ctx.reset_kernel_stats()
            ctx.set_kernel_timing(1)
            msm = wall_ms(torch, lambda: ctx.msm_device(d_p.data_ptr(), d_s.data_ptr(), n, d_pinf.data_ptr()), a.steps, 0)
            ctx.set_kernel_timing(0)
            sclk = ctx.clock_stats()["sclk_ghz"]
            med = {name: statistics.median(ms) for name, ms in ev.items()}
            say(f"2^{lg}: g2_pointwise_mul_device {med_min(ev['g2 pointwise'])} by events, {G2_UNITS['pointwise']} multiplications per point by count = "
                f"{G2_UNITS['pointwise'] * n / (med['g2 pointwise'] * 1e6):.1f} G/s, {med['g2 pointwise'] * 1e6 / n:.1f} ns per point")
            say(f"2^{lg}: g2_scale_device {med_min(ev['g2 scale'])} by events; per-element / one scalar = {med['g2 pointwise'] / med['g2 scale']:.3f} x "
                f"(by count {G2_UNITS['pointwise'] / G2_UNITS['scale']:.3f} x; G1 beside it {med['g1 pointwise'] / med['g1 scale']:.3f} x)")
            say(f"2^{lg}: G1 pointwise_mul_device {med_min(ev['g1 pointwise'])}, scale_device {med_min(ev['g1 scale'])} by events: G2 / G1 = "
                f"{med['g2 pointwise'] / med['g1 pointwise']:.2f} x per element, {med['g2 scale'] / med['g1 scale']:.2f} x with one scalar "
                f"(by count {G2_LIMB['pointwise'] / G1_LIMB['pointwise']:.2f} x in limb products, {G2_UNITS['pointwise'] / G1_UNITS['pointwise']:.2f} x in units)")
            say(f"2^{lg}: g2_fixed_base_mul_device {med_min(ev['g2 fixed'])} by events: pointwise / fixed base = {med['g2 pointwise'] / med['g2 fixed']:.1f} x; "
                f"G1 MSM on the G1 points {med_min(msm)} by the host clock at sclk {sclk:.3f} GHz")
    say("device: %s" % torch.cuda.get_device_name(0))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
