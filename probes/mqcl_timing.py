"""Timing of the exact MQCLE step (gple_mqcl_evolve): ms per Trotter step as the median of GPLE_TIMER_MQCL over calls of a fixed
number of steps after a warm-up call, HBM bytes per step over that time, FFT flops (5 M log2 M per length-M FFT) over that time, and the numpy
restatement's seconds per step on the same box as a baseline (not a result).

    python probes/mqcl_timing.py [--sizes 481,961,1921,3841] [--steps 10] [--reps 5] [--numpy-max 961]
"""
import argparse
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import gaussian_process_liouville_equation_amd as pkg  # noqa: E402
from tests import mqcl_numpy as MN  # noqa: E402

TIMER_MQCL = 5


def state(num_pes, n):
    i = np.arange(n, dtype=np.float64)
    x = (-15.0 * (n - 1 - i) + 15.0 * i) / (n - 1)
    p = ((63.2 - 50.0) * (n - 1 - i) + (63.2 + 50.0) * i) / (n - 1)
    rho = np.zeros((num_pes, num_pes, n, n), dtype=np.complex128)
    rho[0, 0] = np.exp(-(((x[:, None] + 8.0) / 0.158) ** 2 + ((p[None, :] - 63.2) / 3.16) ** 2) / 2.0)
    return x, p, rho


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="481,961,1921,3841")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--numpy-max", type=int, default=961)
    a = ap.parse_args()
    api = pkg.open_api(0)
    api.enable_timing(True)
    print("| n | num_pes | M | ms / step | HBM GB / step | HBM TB/s (of 6.3) | FFT Tflop/s | numpy s / step (baseline) |")
    print("|---|---|---|---|---|---|---|---|")
    for n in [int(v) for v in a.sizes.split(",")]:
        for num_pes in (2, 3):
            model = 1 if num_pes == 2 else 3
            x, p, rho = state(num_pes, n)
            dx_, dp_ = torch.from_numpy(x).cuda(), torch.from_numpy(p).cuda()
            r = torch.from_numpy(rho).cuda()
            ms = []
            for k in range(1 + a.reps):  # call 0 warms up
                api.mqcl_evolve(num_pes, model, dx_, dp_, r, 2000.0, 30.0, 100.0, 2.0 ** -6, a.steps)
                last, _, _ = api.timing(TIMER_MQCL)
                if k:
                    ms.append(last)
            # a call of K steps runs K P passes and K + 1 X passes: per step, the median over K (the extra X pass is 1 / K of a step's X work)
            t = float(np.median(ms)) / a.steps
            M = 2 ** math.ceil(math.log2(2 * n - 1))
            nu = num_pes * (num_pes + 1) // 2
            plane = 16.0 * n * n
            hbm = 4 * 2 * nu * plane  # per step: transpose in, X pass, transpose out, P pass; each reads and writes the nu planes
            flops = 3 * 4 * n * nu * 5.0 * M * math.log2(M)  # per step and row: three shifts (R twice, P once) of four FFTs
            base = ""
            if n <= a.numpy_max:
                bases = MN.Bases(x, model, num_pes)
                t0 = time.perf_counter()
                MN.step(rho, bases, p, 2000.0, 30.0, 100.0, 2.0 ** -6)
                base = f"{time.perf_counter() - t0:.2f}"
            print(f"| {n} | {num_pes} | {M} | {t:.3f} | {hbm / 1e9:.3f} | {hbm / (t * 1e-3) / 1e12:.2f} | {flops / (t * 1e-3) / 1e12:.2f} | {base} |",
                  flush=True)
            del r
            torch.cuda.empty_cache()
    api.close()


if __name__ == "__main__":
    main()
