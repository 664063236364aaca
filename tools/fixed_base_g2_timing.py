#!/usr/bin/env python3
"""The G2 fixed-base batch multiplication on one GPU.  ONE step per invocation (run each under a time limit of its own when the GPU is shared,
tools/README.md), every step in one process:

  --step size --log2 20     msm_bn254_g2_fixed_base_mul_device on 2^20 seeded 256-bit patterns, default c: median and minimum of --steps runs after
                            --warmup, by events on the call's stream and by the host clock around call + synchronise; beside it the G1 fixed-base
                            call on the same scalars, msm_bn254_g2_device on the points just made, and a G1 MSM whose accumulate kernel's clock
                            tells a slow box.  The first points are checked against the Python model.
  --step sweep --log2 20    the same call at c = 8, 10, 11, 12, and per c the table build (a call on ONE scalar with the base changed every time)
  --step group --log2 20    the same call at inv_group = 8, 16, 32 (hooks library, MSM_HIP_FB2_INV_GROUP read when the context is made)
  --step trace --log2 20    --steps calls and nothing else: the process to run under a kernel trace for the split between the two kernels

  python tools/fixed_base_g2_timing.py --step size --log2 20 [--steps 20] [--warmup 3] [--out profiles/fixed_base_g2_timing_mi355x.txt]

Every result line is printed and, with --out, appended to that file."""
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
import fixed_base_cases as fb  # noqa: E402
import fixed_base_g2_cases as fb2  # noqa: E402
from fixed_base_timing import event_ms, med_min, wall_ms  # noqa: E402
from oracle import bn254_oracle as orc  # noqa: E402

MULS_PER_MADD = 33  # 3 Fq products' worth per Fq2 product of the 8M + 2S, and the conversions' share: three times the G1 count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=("size", "sweep", "group", "trace"), required=True)
    ap.add_argument("--log2", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(device=dev)
    s = st.cuda_stream
    n = 1 << a.log2
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    rng = np.random.default_rng(0xF1BA5E2 + a.log2)
    k = rng.integers(0, 1 << 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)  # any 256-bit pattern is a scalar
    d_k = torch.from_numpy(k.view(np.int32)).to(dev)
    d_xy = torch.zeros((n, 32), dtype=torch.int32, device=dev)
    d_inf = torch.zeros(n, dtype=torch.uint8, device=dev)
    gen = fb2.base_words(fb2.GEN)
    want = fb2.expected([orc.words_to_int(w) for w in k[:6]])[0]
    torch.cuda.synchronize()

    def mul_on(ctx, c=0, base=gen, count=n):
        ctx.fixed_base_g2_mul_device(base, d_k.data_ptr(), count, d_xy.data_ptr(), d_inf.data_ptr(), mh.FORM_STD, c, 0, s)

    def check(what):
        torch.cuda.synchronize()
        if not (d_xy[:6].cpu().numpy().view(np.uint32) == want).all():
            raise SystemExit("WRONG RESULT at %s" % (what,))

    if a.step == "group":
        from mopro_msm_hip import testhooks
        for group in (8, 16, 32):
            os.environ["MSM_HIP_FB2_INV_GROUP"] = str(group)
            with testhooks.HooksContext(device=0) as h:
                ev = event_ms(torch, st, lambda: mul_on(h), a.steps, a.warmup)
                check(("inv_group", group))
            say(f"2^{a.log2} scalars, default c, inv_group = {group}: fixed_base_g2_mul_device {med_min(ev)} by events")
        os.environ.pop("MSM_HIP_FB2_INV_GROUP")
    else:
        with mh.MsmContext(device=0) as ctx:
            def mul(c=0, base=gen, count=n):
                mul_on(ctx, c, base, count)

            if a.step == "trace":
                for _ in range(a.steps):
                    mul()
                check("trace")
            elif a.step == "size":
                p = mh.fixed_base_g2_plan()
                ev = event_ms(torch, st, mul, a.steps, a.warmup)
                check("the default c")
                wl = wall_ms(torch, mul, a.steps, a.warmup)
                line = (f"2^{a.log2} scalars, c = {p['window_bits']} ({p['num_windows']} windows, table {p['table_bytes'] / 1e3:.0f} KB, {p['inv_group']} points per "
                        f"inversion, chunks of {p['chunk_points']}): fixed_base_g2_mul_device {med_min(ev)} by events, {med_min(wl)} by the host clock")
                d_xy1 = torch.zeros((n, 16), dtype=torch.int32, device=dev)
                d_inf1 = torch.zeros(n, dtype=torch.uint8, device=dev)
                g1 = fb.base_words(fb.GEN)
                ev1 = event_ms(torch, st, lambda: ctx.fixed_base_mul_device(g1, d_k.data_ptr(), n, d_xy1.data_ptr(), d_inf1.data_ptr(), mh.FORM_STD, 0, 0, s),
                               a.steps, a.warmup)
                line += f"; the G1 fixed-base call {med_min(ev1)} by events = 1/{statistics.median(ev) / statistics.median(ev1):.2f}"
                d_s = torch.from_numpy(orc.gen_scalars(0xB2540032, n).view(np.int32)).to(dev)
                torch.cuda.synchronize()
                m2 = wall_ms(torch, lambda: ctx.msm_g2_device(d_xy.data_ptr(), d_s.data_ptr(), n, d_inf.data_ptr()), a.steps, a.warmup)
                line += f"; G2 MSM on these points {med_min(m2)} by the host clock"
                for _ in range(a.warmup):
                    ctx.msm_device(d_xy1.data_ptr(), d_s.data_ptr(), n, d_inf1.data_ptr())
                ctx.reset_kernel_stats()
                ctx.set_kernel_timing(1)
                m1 = wall_ms(torch, lambda: ctx.msm_device(d_xy1.data_ptr(), d_s.data_ptr(), n, d_inf1.data_ptr()), a.steps, 0)
                ctx.set_kernel_timing(0)
                line += f"; G1 MSM on the G1 points {med_min(m1)} at sclk {ctx.clock_stats()['sclk_ghz']:.3f} GHz"
                say(line)
            else:
                other = [fb2.base_words(fb2.g2.mul(fb2.GEN, 7 + i)) for i in range(a.steps + a.warmup + 1)]
                for c in (8, 10, 11, 12):
                    p = mh.fixed_base_g2_plan(c)
                    mul(c)
                    ev = event_ms(torch, st, lambda: mul(c), a.steps, a.warmup)
                    check(("c", c))
                    it = iter(other)
                    build = event_ms(torch, st, lambda: mul(c, next(it), 1), a.steps, a.warmup)  # the base changes every time: table build + one chain
                    count = p["num_windows"] * MULS_PER_MADD
                    say(f"2^{a.log2} scalars, c = {c}: {p['num_windows']} windows (<= {count} field multiplications per point in additions), table "
                        f"{p['table_entries']} entries = {p['table_bytes'] / 1e3:.0f} KB; fixed_base_g2_mul_device {med_min(ev)} by events; table build + one "
                        f"scalar, the host's subgroup check of the new base included, {med_min(build)}")
    say("device: %s" % torch.cuda.get_device_name(0))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
