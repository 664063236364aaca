#!/usr/bin/env python3
"""The G2 group transform on one GPU, the whole sweep in one process (run it under a time limit when the GPU is shared, tools/README.md):

  per size 2^12, 2^16, 2^18, 2^20 (--log2 12,16,18,20): msm_bn254_g2_fft_device forward and inverse, batch 1 and 3, median and minimum of --steps
      calls after --warmup, by events on the call's stream (the working array is refilled from the source before every call, outside the
      events); beside them, in the same process: msm_bn254_g2_pointwise_mul_device on n / 2 points and msm_bn254_g2_scale_device on n points --
      the kernels a transform is made of -- and msm_bn254_g1_device on n G1 points with the accumulate kernel's shader clock (a slow box shows
      there, as the siblings print it).  Reported: the ratio of every transform to its yardstick,
          forward:  (log n - 1) x pointwise(n / 2)          inverse:  (log n - 1) x pointwise(n / 2) + scale(n)
      times the batch, next to the ratio the count per butterfly predicts: a ladder-stage butterfly is 4 893 / 4 830 of a point's
      multiplication and the first stage's is 82 / 4 830 (g2_fft_bn254.hpp), so
          forward:  ((log n - 1) x 4 893 + 82) / ((log n - 1) x 4 830)
      and the inverse the same over a yardstick that already holds its 1/n pass; the bit-reversal sweep is in neither.

  python tools/g2_fft_timing.py [--batches 1,3] [--steps 5] [--warmup 1] [--out profiles/g2_fft_timing_mi355x.txt]

The points are tau^j * H made by the powers and the G2 fixed-base calls, so both transforms have a closed form per index: forward out[i] =
(tau^n - 1) / (tau w^i - 1) * H, inverse out[i] = L_i(tau) * H; the first and last three outputs of every array of the last call are checked
word for word against the model of tools/fixed_base_g2_cases.py.  Every result line is printed and, with --out, appended."""
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
import g2_fft_cases as gc  # noqa: E402
from fixed_base_timing import event_ms, med_min, wall_ms  # noqa: E402
from g1_fft_timing import closed_form  # noqa: E402  (the logarithm of output i: the group does not enter)

fb2, R = gc.fb2, gc.R
orc = gc.g1c.orc
UNITS_LADDER, UNITS_FIRST, UNITS_POINT = 4893, 82, 4830  # g2_fft_bn254.hpp, g2_pointwise_mul_bn254.hpp


def predicted(lg, inverse, m_pw, m_sc):
    """the ratio to the yardstick that the count per butterfly predicts, from the measured parts of the yardstick"""
    ladder = (lg - 1) * m_pw
    extra = ladder * (UNITS_LADDER - UNITS_POINT) / UNITS_POINT + m_pw * UNITS_FIRST / UNITS_POINT
    yard = ladder + (m_sc if inverse else 0.0)
    return (yard + extra) / yard


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", default="12,16,18,20")
    ap.add_argument("--batches", default="1,3")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch-budget-s", type=float, default=60.0, help="a batch above 1 is skipped where its calls would take longer than this in all")
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

    sizes = [int(v) for v in a.log2.split(",") if v]
    batches = [int(v) for v in a.batches.split(",") if v]
    nmax = max(batches) << max(sizes)
    tau = gc.logs(0x7A0F2, 1)[0]
    rng = np.random.default_rng(0x6F172)
    d_k = torch.from_numpy(rng.integers(0, 1 << 32, size=(nmax, 8), dtype=np.uint64).astype(np.uint32).view(np.int32)).to(dev)  # the yardstick's scalars
    d_pow = torch.zeros((nmax, 8), dtype=torch.int32, device=dev)
    d_src = torch.zeros((nmax, 32), dtype=torch.int32, device=dev)
    d_sinf = torch.zeros(nmax, dtype=torch.uint8, device=dev)
    d_xy = torch.zeros((nmax, 32), dtype=torch.int32, device=dev)
    d_inf = torch.zeros(nmax, dtype=torch.uint8, device=dev)
    n1 = 1 << max(sizes)
    d_s = torch.from_numpy(orc.gen_scalars(0x6F182, n1).view(np.int32)).to(dev)
    d_g1 = torch.zeros((n1, 16), dtype=torch.int32, device=dev)  # the G1 MSM's points, for the clock line
    d_g1inf = torch.zeros(n1, dtype=torch.uint8, device=dev)
    gen1 = np.concatenate([orc.int_to_words(1), orc.int_to_words(2)])
    gen2 = fb2.base_words(gc.GEN)
    one = gc.logs(0x6F192, 1)[0]
    torch.cuda.synchronize()

    def transform_ms(ctx, lg, batch, flags):
        """event times of `steps` transforms; the working array is the source again before each"""
        pts = batch << lg
        ms = []
        for it in range(a.warmup + a.steps):
            with torch.cuda.stream(st):
                d_xy[:pts].copy_(d_src[:pts])
                d_inf[:pts].copy_(d_sinf[:pts])
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            ctx.g2_fft_device(d_xy.data_ptr(), d_inf.data_ptr(), lg, batch, flags, stream=s)
            e1.record(st)
            e1.synchronize()
            if it >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        n = 1 << lg
        at = [b * n + i for b in range(batch) for i in (0, 1, 2, n - 3, n - 2, n - 1)]
        got = (d_xy[at].cpu().numpy().view(np.uint32), d_inf[at].cpu().numpy())
        want = fb2.expected([closed_form(tau, lg, p // n, p % n, bool(flags & gc.INVERSE)) for p in at])
        if not ((got[0] == want[0]).all() and (got[1] == want[1]).all()):
            raise SystemExit("WRONG RESULT at 2^%d batch %d flags %d" % (lg, batch, flags))
        return ms

    with mh.MsmContext(device=0) as ctx:
        ctx.fr_powers_device(tau, d_pow.data_ptr(), nmax, stream=s)
        ctx.fixed_base_g2_mul_device(gen2, d_pow.data_ptr(), nmax, d_src.data_ptr(), d_sinf.data_ptr(), stream=s)  # Q_j = tau^j * H
        ctx.fixed_base_mul_device(gen1, d_pow.data_ptr(), n1, d_g1.data_ptr(), d_g1inf.data_ptr(), stream=s)
        st.synchronize()
        say("plan at 2^%d: %s" % (max(sizes), mh.g2_fft_plan(max(sizes))))
        for lg in sizes:
            n = 1 << lg
            pw = event_ms(torch, st, lambda: ctx.g2_pointwise_mul_device(d_src.data_ptr(), d_k.data_ptr(), n // 2, d_xy.data_ptr(), d_inf.data_ptr(),
                                                                         d_sinf.data_ptr(), stream=s), a.steps, a.warmup)
            sc = event_ms(torch, st, lambda: ctx.g2_scale_device(d_src.data_ptr(), one, n, d_xy.data_ptr(), d_inf.data_ptr(), d_sinf.data_ptr(), stream=s),
                          a.steps, a.warmup)
            for _ in range(a.warmup):
                ctx.msm_device(d_g1.data_ptr(), d_s.data_ptr(), n, d_g1inf.data_ptr())
            ctx.reset_kernel_stats()
            ctx.set_kernel_timing(1)
            msm = wall_ms(torch, lambda: ctx.msm_device(d_g1.data_ptr(), d_s.data_ptr(), n, d_g1inf.data_ptr()), a.steps, 0)
            ctx.set_kernel_timing(0)
            sclk = ctx.clock_stats()["sclk_ghz"]
            m_pw, m_sc = statistics.median(pw), statistics.median(sc)
            yard = {0: (lg - 1) * m_pw, gc.INVERSE: (lg - 1) * m_pw + m_sc}
            say(f"2^{lg}: g2_pointwise_mul_device on n/2 {med_min(pw)}, g2_scale_device on n {med_min(sc)} by events; G1 MSM on n {med_min(msm)} by the host "
                f"clock at sclk {sclk:.3f} GHz; yardsticks: forward {yard[0]:.4f} ms, inverse {yard[gc.INVERSE]:.4f} ms")
            for flags, name in ((0, "forward"), (gc.INVERSE, "inverse")):
                for batch in batches:
                    if batch > 1 and batch * yard[flags] * (a.steps + a.warmup) > a.batch_budget_s * 1e3:
                        say(f"2^{lg}: g2_fft_device {name} batch {batch} skipped: its calls would take more than {a.batch_budget_s:.0f} s")
                        continue
                    ms = transform_ms(ctx, lg, batch, flags)
                    m = statistics.median(ms)
                    say(f"2^{lg}: g2_fft_device {name} batch {batch} {med_min(ms)} by events = {m * 1e6 / (batch * n):.1f} ns per point; "
                        f"/ (batch x yardstick) = {m / (batch * yard[flags]):.3f}; by the count {predicted(lg, bool(flags), m_pw, m_sc):.3f}")
    say("device: %s" % torch.cuda.get_device_name(0))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
