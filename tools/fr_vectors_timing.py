#!/usr/bin/env python3
"""The scalar-vector calls on one GPU, the whole sweep in one process (run it under a time limit when the GPU is shared, tools/README.md):

  per size 2^16, 2^18, 2^20, 2^22 (--log2 16,18,20,22): msm_bn254_fr_powers_device, _batch_inverse_device, _lagrange_device and _lincomb_device
      (three terms), median and minimum of --steps calls after --warmup, by events on the call's stream; beside them, in the same process, the
      yardsticks the project already has: msm_bn254_fr_mul_sub_scale_device (3 field multiplications per element), one forward transform of the
      size, the G1 fixed-base call the scalars feed, and the hipMemcpy of n x 32 bytes from pinned host memory that the calls replace.
  at 2^20 (--group-log2): _batch_inverse_device at inv_group = 4, 8, 16, 32 (hooks library, MSM_HIP_FRV_INV_GROUP read when the context is made)

  python tools/fr_vectors_timing.py [--steps 20] [--warmup 3] [--out profiles/fr_vectors_timing_mi355x.txt]

The first and last elements of every result are checked against the Python yardstick.  Every result line is printed and, with --out, appended."""
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
import bn254_fr_vectors_py as frv  # noqa: E402
import fixed_base_cases as fb  # noqa: E402
from fixed_base_timing import event_ms, med_min  # noqa: E402

R = frv.R
# field multiplications per element, by count (fr_vectors_bn254.hpp): the chain's 4 (zero test, product up, two on the way down) + 381 / inv_group
# for the shared inversion; the power walk's 1 + (6 + the wavefront's bits) / 16; Lagrange's 6 + the inversion's share; lincomb's 3 + 1
MULS_INV = 381  # 254 squarings + 127 multiplications of r - 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", default="16,18,20,22")
    ap.add_argument("--group-log2", type=int, default=20)
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

    def head_tail(t, n, k=3):
        torch.cuda.synchronize()
        return frv.from_words(torch.cat([t[:k], t[n - k:n]]).cpu().numpy().view(np.uint32))

    def must(what, got, want):
        if got != want:
            raise SystemExit("WRONG RESULT at %s" % (what,))

    tau, scale, ka, kb, kc = frv.patterns(0x71A1, 5)
    plan = mh.fr_vector_plan()
    G = plan["inv_group"]
    say("plan: %s" % plan)
    sizes = [int(v) for v in a.log2.split(",") if v]
    nmax = 1 << max(sizes + [a.group_log2])
    rng = np.random.default_rng(0x71A2)
    h_x = rng.integers(0, 1 << 32, size=(nmax, 8), dtype=np.uint64).astype(np.uint32)
    d_x = torch.from_numpy(h_x.view(np.int32)).to(dev)
    d_y = torch.from_numpy(np.roll(h_x, 1, axis=0).view(np.int32)).to(dev)
    d_z = torch.from_numpy(np.roll(h_x, 2, axis=0).view(np.int32)).to(dev)
    d_out = torch.zeros((nmax, 8), dtype=torch.int32, device=dev)
    h_pin = torch.from_numpy(h_x.view(np.int32)).pin_memory()
    ends = lambda n: (0, 1, 2, n - 3, n - 2, n - 1)
    pats = lambda n, shift=0: frv.from_words(np.stack([h_x[(i - shift) % nmax] for i in ends(n)]))  # d_x, d_y, d_z at the checked places
    torch.cuda.synchronize()

    with mh.MsmContext(device=0) as ctx:
        for lg in sizes:
            n = 1 << lg
            ev = {}
            ev["powers"] = event_ms(torch, st, lambda: ctx.fr_powers_device(tau, d_out.data_ptr(), n, scale=scale, stream=s), a.steps, a.warmup)
            must(("powers", lg), head_tail(d_out, n), [scale * pow(tau, i, R) % R for i in ends(n)])
            ev["batch_inverse"] = event_ms(torch, st, lambda: ctx.fr_batch_inverse_device(d_x.data_ptr(), d_out.data_ptr(), n, stream=s), a.steps, a.warmup)
            must(("inverse", lg), head_tail(d_out, n), frv.batch_inverse(pats(n)))
            ev["lagrange"] = event_ms(torch, st, lambda: ctx.fr_lagrange_device(tau, lg, d_out.data_ptr(), stream=s), a.steps, a.warmup)
            w, zn = frv.root_of_unity(lg), (pow(tau, n, R) - 1) * frv.inverse(n) % R
            must(("lagrange", lg), head_tail(d_out, n), [zn * pow(w, i, R) * frv.inverse(tau - pow(w, i, R)) % R for i in ends(n)])
            ev["lincomb"] = event_ms(torch, st, lambda: ctx.fr_lincomb_device(d_x.data_ptr(), d_out.data_ptr(), n, ka, d_y.data_ptr(), kb, d_z.data_ptr(), kc,
                                                                              stream=s), a.steps, a.warmup)
            must(("lincomb", lg), head_tail(d_out, n), frv.lincomb(pats(n), ka, pats(n, 1), kb, pats(n, 2), kc))
            # the yardsticks
            ev["mul_sub_scale"] = event_ms(torch, st, lambda: ctx.fr_mul_sub_scale_device(d_x.data_ptr(), d_y.data_ptr(), d_z.data_ptr(), d_out.data_ptr(), n,
                                                                                          k=ka, stream=s), a.steps, a.warmup)
            ev["ntt forward"] = event_ms(torch, st, lambda: ctx.ntt_device(d_out.data_ptr(), lg, stream=s), a.steps, a.warmup)
            with torch.cuda.stream(st):
                ev["hipMemcpy H2D"] = event_ms(torch, st, lambda: d_out[:n].copy_(h_pin[:n], non_blocking=True), a.steps, a.warmup)
            d_xy = torch.zeros((n, 16), dtype=torch.int32, device=dev)
            d_inf = torch.zeros(n, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            g1 = fb.base_words(fb.GEN)
            ev["G1 fixed-base mul"] = event_ms(torch, st, lambda: ctx.fixed_base_mul_device(g1, d_x.data_ptr(), n, d_xy.data_ptr(), d_inf.data_ptr(), stream=s),
                                               max(3, a.steps // 4), 1)
            del d_xy, d_inf
            base = statistics.median(ev["mul_sub_scale"])
            copy = statistics.median(ev["hipMemcpy H2D"])
            wave_bits = max(lg - 10, 0) / 2  # set bits of a wavefront's number, on average
            counts = {"powers": 1 + (6 + wave_bits) / 16, "batch_inverse": 4 + MULS_INV / G, "lagrange": 6 + (MULS_INV + 6 + max(lg - 6, 0) / 2) / G,
                      "lincomb": 4, "mul_sub_scale": 3}
            for name, ms in ev.items():
                extra = ""
                if name in counts:
                    extra = "; %.2f multiplications per element by count = %.2f x mul_sub_scale's, measured %.2f x" % (
                        counts[name], counts[name] / 3, statistics.median(ms) / base)
                if name in ("powers", "batch_inverse", "lagrange", "lincomb"):
                    extra += "; the copy it replaces takes %.2f x as long" % (copy / statistics.median(ms))
                say(f"2^{lg}: {name} {med_min(ms)} by events{extra}")

    from mopro_msm_hip import testhooks
    n = 1 << a.group_log2
    for group in (4, 8, 16, 32):
        os.environ["MSM_HIP_FRV_INV_GROUP"] = str(group)
        with testhooks.HooksContext(device=0) as h:
            ms = event_ms(torch, st, lambda: h.fr_batch_inverse_device(d_x.data_ptr(), d_out.data_ptr(), n, stream=s), a.steps, a.warmup)
            must(("inv_group", group), head_tail(d_out, n), frv.batch_inverse(pats(n)))
        say(f"2^{a.group_log2}, inv_group = {group}: batch_inverse {med_min(ms)} by events; {4 + MULS_INV / group:.1f} multiplications per element by count")
    os.environ.pop("MSM_HIP_FRV_INV_GROUP")
    say("device: %s" % torch.cuda.get_device_name(0))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
