"""Time of the smoothed phase-space density (gple_hop_smooth; DESIGN.md §17, "The ensemble in phase space, smoothed") on the throughput ensembles
of §17: 2^20 DAC trajectories (two levels, 4 planes) and 2^20 TSAC (three levels, 9 planes) on 256 x 256 with h = 1.5 d, in one process:
GPLE_TIMER_HOP_SMOOTH, the three kernels of a call, as the median (min - max) of `--reps` calls after a warm-up call, in ms and as the fraction
of the 78.6 TFLOP/s fp64 MFMA peak at 2 P n_x n_p n_used flop.  Beside it, for orientation, gple_hop_bin + gple_hop_density on the same
ensemble (GPLE_TIMER_HOP_BIN; the density kernel has no timer and is a pass over the grid).

The yardstick is the library's own GEMM on the same shape in the same run: the operands A_q[k, i] = u_qi g_x(x_k - x_i) and
B[i, j] = g_p(p_j - p_i) are written out by throw-away torch kernels, `--chunk` trajectories at a time, and contracted per plane with
gple_debug_gemm, accumulated over the chunks (beta = 1).  The weights of the coherence planes are taken from the diabatic amplitudes: the
time of a GEMM does not depend on the values.  gple_debug_gemm stages host operands and has no timer, so the probe reports its wall clock,
staging included, and the kernels alone are read from a kernel trace of the same process:
    timeout 900 rocprofv3 --kernel-trace --output-format csv -d trace -- python probes/hop_smooth_timing.py
    python probes/hop_smooth_timing.py --kernel-trace trace/<host>/<pid>_kernel_trace.csv
The second command touches no GPU: it sums the GEMM launches of every yardstick pass and the three kernels of every smooth call.
Prints one JSON line.

    timeout 900 python probes/hop_smooth_timing.py [--trajectories 1048576] [--reps 5] [--yardstick-passes 3] [--chunk 131072]
"""
import argparse
import csv
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MASS, X0, P0, BOUND, SEED, N_GRID, PEAK = 2000.0, -4.0, 10.0, 6.0, 7, 256, 78.6e12
ENSEMBLES = {"dac": dict(N=2, model=1, dt=2.0, steps=300, surface0=0), "tsac": dict(N=3, model=3, dt=4.0, steps=150, surface0=1)}


def spread(ms):
    return dict(ms=float(np.median(ms)), ms_min=float(min(ms)), ms_max=float(max(ms)))


def grid_of(state):
    x, p = state[0].cpu().numpy(), state[1].cpu().numpy()
    return (float(x.min()), float(np.ptp(x)) / (N_GRID - 1), N_GRID, float(p.min()), float(np.ptp(p)) / (N_GRID - 1), N_GRID)


def yardstick(api, state, grid, h, N, chunk):
    """one pass: the operands of every chunk written out, one gple_debug_gemm per plane and chunk -> seconds of the GEMM calls (staging included)"""
    import torch

    x, p, b, surface, status = state
    n = x.shape[0]
    running = (status == 0).to(torch.float64)
    planes = [running * (surface == a).to(torch.float64) for a in range(N)]
    for a in range(N):
        for c in range(a + 1, N):
            z = b[:, a] * torch.conj(b[:, c])
            planes += [running * z.real, running * z.imag]
    xk = grid[0] + grid[1] * torch.arange(N_GRID, dtype=torch.float64, device=x.device)
    pj = grid[3] + grid[4] * torch.arange(N_GRID, dtype=torch.float64, device=x.device)
    fn = api.lib.gple_debug_gemm
    fn.restype = ctypes.c_int
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    out = [np.zeros((N_GRID, N_GRID)) for _ in planes]  # C(m, n) at m + n ldc: [p line][x line]
    seconds = 0.0
    for i0 in range(0, n, chunk):
        i1 = min(i0 + chunk, n)
        K = i1 - i0
        g_x = torch.exp(-0.5 * ((xk[None, :] - x[i0:i1, None]) / h[0]) ** 2)  # (K, n_x): element (m, k) at m + k lda
        B = torch.exp(-0.5 * ((pj[None, :] - p[i0:i1, None]) / h[1]) ** 2).cpu().numpy()
        for q, u in enumerate(planes):
            A = (u[i0:i1, None] * g_x).cpu().numpy()
            t0 = time.perf_counter()
            rc = fn(api.ctx, ptr(A), ctypes.c_long(N_GRID), 0, ptr(B), ctypes.c_long(N_GRID), 0, ptr(out[q]), ctypes.c_long(N_GRID), 0, N_GRID, N_GRID, K,
                    ctypes.c_double(1.0), ctypes.c_double(1.0), 0, 0, 0)
            seconds += time.perf_counter() - t0
            assert rc == 0, rc
    return seconds, out


def measure(a):
    import gaussian_process_liouville_equation_amd as pkg
    from gaussian_process_liouville_equation_amd import _capi

    api = pkg.open_api(0)
    api.enable_timing(True)
    rows = []
    try:
        for name, e in ENSEMBLES.items():
            N, model = e["N"], e["model"]
            state = api.hop_sample(N, model, a.trajectories, SEED, X0, P0, 1.0 / (2.0 * P0 / 20.0), P0 / 20.0, e["surface0"], device_out=True)
            state = api.hop_evolve(N, model, state, SEED, MASS, e["dt"], 0, e["steps"], -BOUND, BOUND)
            api.synchronize()
            grid = grid_of(state)
            h = (1.5 * grid[1], 1.5 * grid[4])
            smooth_ms, bin_ms = [], []
            for k in range(1 + a.reps):  # call 0 of either warms up; the two take turns
                rho, (used, nonfinite) = api.hop_smooth(N, model, state, grid, h, a.trajectories)
                last = api.timing(_capi.TIMER_HOP_SMOOTH)[0]
                acc = api.hop_bin(N, model, state, grid)
                api.hop_density(N, grid, acc, a.trajectories)
                last_bin = api.timing(_capi.TIMER_HOP_BIN)[0]
                if k:
                    smooth_ms.append(last)
                    bin_ms.append(last_bin)
            flop = 2.0 * N * N * N_GRID * N_GRID * used
            one, two = spread(smooth_ms), spread(bin_ms)
            row = dict(ensemble=name, planes=N * N, used=used, nonfinite=nonfinite, smooth=one, of_peak=flop / (one["ms"] * 1e-3) / PEAK, bin=two)
            if a.yardstick_passes:
                passes = []
                for _ in range(1 + a.yardstick_passes):  # pass 0 warms up
                    seconds, out = yardstick(api, state, grid, h, N, a.chunk)
                    passes.append(1e3 * seconds)
                row["yardstick_wall"] = spread(passes[1:])
                row["yardstick_launches_per_pass"] = N * N * -(-a.trajectories // a.chunk)
                # the populations of the two agree: the yardstick contracts what the call contracts
                s = 1.0 / (a.trajectories * 2.0 * np.pi * h[0] * h[1])
                field = rho.cpu().numpy()
                for q in range(N):
                    assert np.allclose(s * out[q].T, field[q, q].real, rtol=1e-9, atol=1e-12 * field[q, q].real.max()), (name, q)
            rows.append(row)
    finally:
        api.close()
    print(json.dumps(dict(probe="hop_smooth_timing", trajectories=a.trajectories, reps=a.reps, chunk=a.chunk, grid=N_GRID, rows=rows)))


def from_trace(a):
    """the kernels alone, from the kernel trace of a run of this probe with its defaults' structure: per ensemble 1 + reps smooth calls, then
    1 + passes yardstick passes of planes x chunks GEMM launches"""
    spans = []
    with open(a.kernel_trace, newline="") as f:
        for r in csv.DictReader(f):
            spans.append((int(r["Start_Timestamp"]), r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6))
    spans.sort()
    smooth = [ms for _, name, ms in spans if "hop_smooth_kernel" in name]
    whole = {}
    for part in ("hop_smooth_terms_kernel", "hop_smooth_kernel", "hop_smooth_finish_kernel"):
        whole[part] = [ms for _, name, ms in spans if part in name]
    gemm = [ms for _, name, ms in spans if "gemm" in name.lower() and "hop_smooth" not in name]
    rows, at_s, at_g = [], 0, 0
    chunks = -(-a.trajectories // a.chunk)
    for name, e in ENSEMBLES.items():
        calls = slice(at_s + 1, at_s + 1 + a.reps)
        three = [sum(v) for v in zip(*(whole[part][calls] for part in whole))]
        per = e["N"] ** 2 * chunks
        passes = [sum(gemm[at_g + k * per:at_g + (k + 1) * per]) for k in range(1, 1 + a.yardstick_passes)]
        rows.append(dict(ensemble=name, contraction=spread(smooth[calls]), three_kernels=spread(three), yardstick_gemm=spread(passes), launches_per_pass=per))
        at_s += 1 + a.reps
        at_g += (1 + a.yardstick_passes) * per
    assert at_s == len(smooth) and at_g == len(gemm), (at_s, len(smooth), at_g, len(gemm))
    for r in rows:
        r["within_yardstick_spread"] = bool(r["three_kernels"]["ms"] <= r["yardstick_gemm"]["ms"] + r["yardstick_gemm"]["ms_max"] - r["yardstick_gemm"]["ms_min"])
    print(json.dumps(dict(probe="hop_smooth_timing", source="kernel trace", rows=rows)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trajectories", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--yardstick-passes", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=1 << 17)
    ap.add_argument("--kernel-trace", default=None)
    a = ap.parse_args()
    if a.kernel_trace:
        from_trace(a)
    else:
        measure(a)


if __name__ == "__main__":
    main()
