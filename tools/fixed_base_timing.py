#!/usr/bin/env python3
"""The G1 fixed-base batch multiplication on one GPU.  ONE step per invocation (run each under a time limit of its own when the GPU is shared,
tools/README.md), every step in one process:

  --step size --log2 20     msm_bn254_g1_fixed_base_mul_device on 2^20 seeded 256-bit patterns, default c: median and minimum of --steps runs after
                            --warmup, by events on the call's stream and by the host clock around call + synchronise; beside it, by the same host
                            clock, the hooks library's msm_bn254_g1_generate_device at the same n (254 one-bit windows and one inversion per point:
                            how such points were made before) and msm_bn254_g1_device on the points just made (the accumulate kernel's clock tells
                            a slow box).  The first points are checked against the oracle, the hook's against the call on the hook's scalars.
  --step sweep --log2 20    the same call at c = 6, 8, 10, 12, and per c the table build (a call on ONE scalar with the base changed every time)

  python tools/fixed_base_timing.py --step size --log2 20 [--steps 20] [--warmup 3] [--out profiles/fixed_base_timing_mi355x.txt]

Every result line is printed and, with --out, appended to that file."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "gpu-acceleration_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import mopro_msm_hip as mh  # noqa: E402
import fixed_base_cases as fb  # noqa: E402
from oracle import bn254_oracle as orc  # noqa: E402

MULS_PER_MADD = 11  # 8M + 2S and the conversions' share: the count DESIGN.md 9e argues with


def event_ms(torch, stream, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    stream.synchronize()
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def wall_ms(torch, fn, steps, warmup):
    """fn blocks, or is followed by a synchronise: host clock around both"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def med_min(ms):
    return "%.4f ms (min %.4f)" % (statistics.median(ms), min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=("size", "sweep"), required=True)
    ap.add_argument("--log2", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from mopro_msm_hip import testhooks
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(device=dev)
    s = st.cuda_stream
    n = 1 << a.log2
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    rng = np.random.default_rng(0xF1BA5E + a.log2)
    k = rng.integers(0, 1 << 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)  # any 256-bit pattern is a scalar
    d_k = torch.from_numpy(k.view(np.int32)).to(dev)
    d_xy = torch.zeros((n, 16), dtype=torch.int32, device=dev)
    d_inf = torch.zeros(n, dtype=torch.uint8, device=dev)
    gen = fb.base_words(fb.GEN)
    torch.cuda.synchronize()
    with mh.MsmContext(device=0) as ctx:
        def mul(c=0, base=gen, count=n):
            ctx.fixed_base_mul_device(base, d_k.data_ptr(), count, d_xy.data_ptr(), d_inf.data_ptr(), mh.FORM_STD, c, 0, s)

        def check(c):
            torch.cuda.synchronize()
            got = d_xy[:6].cpu().numpy().view(np.uint32)
            want = fb.expected([orc.words_to_int(w) for w in k[:6]])[0]
            if not (got == want).all():
                raise SystemExit("WRONG RESULT at c = %d" % c)

        if a.step == "size":
            p = mh.fixed_base_plan()
            ev = event_ms(torch, st, mul, a.steps, a.warmup)
            check(0)
            wl = wall_ms(torch, mul, a.steps, a.warmup)
            line = (f"2^{a.log2} scalars, c = {p['window_bits']} ({p['num_windows']} windows, table {p['table_bytes'] / 1e3:.0f} KB, {p['inv_group']} points per "
                    f"inversion): fixed_base_mul_device {med_min(ev)} by events, {med_min(wl)} by the host clock")
            with testhooks.HooksContext(device=0) as h:
                hk = wall_ms(torch, lambda: h.generate_device(0xB2540031, 0, n, d_xy.data_ptr(), None), a.steps, a.warmup)
                hook_pts = d_xy[:64].cpu().numpy().view(np.uint32).copy()
            hook_k = orc.gen_scalars(0xB2540031, 64, nonzero=True)
            if not (hook_pts == fb.expected([orc.words_to_int(w) for w in hook_k])[0]).all():
                raise SystemExit("WRONG RESULT: the hook's points")
            ratio = statistics.median(hk) / statistics.median(wl)
            line += f"; hooks generate_device {med_min(hk)} by the host clock = {ratio:.2f}x"
            mul()  # the points of k again: bases of the MSM beside it
            torch.cuda.synchronize()
            d_s = torch.from_numpy(orc.gen_scalars(0xB2540032, n).view(np.int32)).to(dev)
            for _ in range(a.warmup):
                ctx.msm_device(d_xy.data_ptr(), d_s.data_ptr(), n, d_inf.data_ptr())
            ctx.reset_kernel_stats()
            ctx.set_kernel_timing(1)
            mm = wall_ms(torch, lambda: ctx.msm_device(d_xy.data_ptr(), d_s.data_ptr(), n, d_inf.data_ptr()), a.steps, 0)
            ctx.set_kernel_timing(0)
            line += f"; G1 MSM on these points {med_min(mm)} at sclk {ctx.clock_stats()['sclk_ghz']:.3f} GHz"
            say(line)
        else:
            other = [fb.base_words(fb.point(7 + i)) for i in range(a.steps + a.warmup + 1)]
            for c in (6, 8, 10, 12):
                p = mh.fixed_base_plan(c)
                mul(c)
                ev = event_ms(torch, st, lambda: mul(c), a.steps, a.warmup)
                check(c)
                it = iter(other)
                build = event_ms(torch, st, lambda: mul(c, next(it), 1), a.steps, a.warmup)  # the base changes every time: table build + one group
                count = p["num_windows"] * MULS_PER_MADD
                say(f"2^{a.log2} scalars, c = {c}: {p['num_windows']} windows (<= {count} field multiplications per point in additions), table "
                    f"{p['table_entries']} entries = {p['table_bytes'] / 1e3:.0f} KB; fixed_base_mul_device {med_min(ev)} by events; table build + one "
                    f"scalar {med_min(build)}")
    say("device: %s" % torch.cuda.get_device_name(0))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
