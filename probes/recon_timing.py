"""Timing of the grid reconstruction (gple_grid_reconstruct) against the route the library had before it for the same result:
gple_nlml_predict on the nx * np explicit grid points of every fitted plane, device pointers, prediction only (GPLE_TIMER_PREDICT: its
Gram, factorisation and solve are left out, as gple_nlml_weights' are on the new side).  The library's device events on the context's stream
(GPLE_TIMER_RECON: tables + contraction + final sum) read after a synchronise, median of --reps after a warm-up, the two routes alternated in
one process.  Prints the markdown table of §13: ms
with and without the stored prediction, the old route's ms, the ratio, and the new route's share of max(flops / 78.6 TFLOP/s, bytes / 6.3 TB/s).

With --cross a second table for the cross-term kernel (gple_grid_reconstruct_cross, x = (w_d, w_g, a, c, b) with c = --shear): its ms with
and without the stored prediction, the share of its tiles that take the centred (MFMA) form, and its two yardsticks measured in the same
process, alternated — (a) gple_nlml_cross_predict on the explicit points (GPLE_TIMER_PREDICT alone), the only route the library had for this
kernel, and (b) gple_grid_reconstruct at the same n and N, the same contraction without exponentials inside it.  --ax replaces a_x = 1 / SX
in every route (a narrower or wider kernel moves tiles across the range rule |a| max|u| <= 6).

    python probes/recon_timing.py [--sizes 961,1921,3841] [--points 200,1024] [--reps 5] [--no-old] [--cross] [--shear -0.5] [--ax 6.33]
"""
import argparse
import ctypes as C
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import gaussian_process_liouville_equation_amd as pkg  # noqa: E402
from gaussian_process_liouville_equation_amd import _capi  # noqa: E402

PEAK_FLOPS, PEAK_BYTES = 78.6e12, 6.3e12
SX, SP = 0.158, 3.16
HYPER = np.array([1e-3, 0.8, 1.0 / SX, 1.0 / SP])


def state(n):
    i = np.arange(n, dtype=np.float64)
    x = (-15.0 * (n - 1 - i) + 15.0 * i) / (n - 1)
    p = ((63.2 - 50.0) * (n - 1 - i) + (63.2 + 50.0) * i) / (n - 1)
    g = lambda cx, cp: np.exp(-(((x[:, None] - cx) / SX) ** 2 + ((p[None, :] - cp) / SP) ** 2) / 2.0)
    rho = np.zeros((2, 2, n, n), dtype=np.complex128)
    rho[0, 0], rho[1, 1] = 0.7 * g(-8.0, 63.2), 0.3 * g(-6.5, 60.0)
    rho[0, 1] = np.sqrt(rho[0, 0].real * rho[1, 1].real) * np.exp(0.5j * (x[:, None] + 8.0))
    rho[1, 0] = np.conj(rho[0, 1])
    return x, p, rho


TIMER_PREDICT, TIMER_RECON = 1, 6


def timed(api, which, fn, reps):
    """median over reps of the milliseconds timer `which` accumulates during one fn() (call 0 warms up)"""
    ms = []
    for k in range(reps + 1):
        before = api.timing(which)[1]
        fn()
        if k:
            ms.append(api.timing(which)[1] - before)
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="961,1921,3841")
    ap.add_argument("--points", default="200,1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-old", action="store_true")
    ap.add_argument("--cross", action="store_true")
    ap.add_argument("--shear", type=float, default=-0.5)
    ap.add_argument("--ax", type=float, default=HYPER[2])
    a = ap.parse_args()
    hyper = HYPER.copy()
    hyper[2] = a.ax
    hyper5 = np.array([hyper[0], hyper[1], hyper[2], a.shear, hyper[3]])
    cross_rows = []
    api = pkg.open_api(0)
    api.enable_timing(True)
    lib = api.lib
    print("| n | N | reconstruct + pred ms | reconstruct ms | nlml_predict route ms | old / new | bound | share of bound (with pred) |")
    print("|---|---|---|---|---|---|---|---|")
    for n in [int(v) for v in a.sizes.split(",")]:
        x, p, rho = state(n)
        planes_v = [rho[0, 0].real, rho[0, 1].real, rho[0, 1].imag, rho[1, 1].real]
        dx, dp = (x[-1] - x[0]) / n, (p[-1] - p[0]) / n
        dr, dxs, dps = torch.from_numpy(rho).cuda(), torch.from_numpy(x).cuda(), torch.from_numpy(p).cuda()
        grid_pts = torch.stack(torch.meshgrid(dxs, dps, indexing="ij"), dim=-1).reshape(-1, 2).contiguous()
        mean = torch.empty(n * n, dtype=torch.float64, device="cuda")
        for N in [int(v) for v in a.points.split(",")]:
            rng = np.random.default_rng(n + N)
            host, dev = [], []
            for v in planes_v:
                w = np.abs(v).ravel()
                cells = np.sort(rng.choice(w.size, size=N, replace=False, p=w / w.sum()))
                X = np.ascontiguousarray(np.stack([x[cells // n], p[cells % n]], axis=1))
                y = v.ravel()[cells].copy()
                b = api.nlml_weights(hyper, X, y)
                host.append((X, y))
                dev.append((hyper, torch.from_numpy(X).cuda(), torch.from_numpy(b).cuda()))
            t_pred = timed(api, TIMER_RECON, lambda: api.grid_reconstruct(2, 1, dr, dxs, dps, 2000.0, dx, dp, dev, None, want_pred=True), a.reps)
            t_sums = timed(api, TIMER_RECON, lambda: api.grid_reconstruct(2, 1, dr, dxs, dps, 2000.0, dx, dp, dev, None, want_pred=False), a.reps)

            def old():
                for X, y in host:  # the training set is a host argument of gple_nlml_predict; grid points and result stay on the device
                    api._check(lib.gple_nlml_predict(api.ctx, _capi._ptr(hyper), _capi._ptr(X), _capi._ptr(y), N, C.cast(grid_pts.data_ptr(), _capi._dp), n * n,
                                                     _capi.IO_DEVICE, C.cast(mean.data_ptr(), _capi._dp)))
            t_old = float("nan") if a.no_old else timed(api, TIMER_PREDICT, old, a.reps)
            npad, rows = 4 * (N + 15) // 16 * 16, (n + 63) // 64 * 64
            flops = 2.0 * n * n * npad
            byts = 16.0 * n * n * 3 + 8.0 * n * n * 4 + 8.0 * 2 * rows * npad * 2  # elements read, planes stored, tables written and read once
            t_f, t_b = flops / PEAK_FLOPS * 1e3, byts / PEAK_BYTES * 1e3
            print(f"| {n} | {N} | {t_pred:.3f} | {t_sums:.3f} | {t_old:.2f} | {t_old / t_pred:.1f} | {'MFMA' if t_f > t_b else 'HBM'} {max(t_f, t_b):.3f} ms | "
                  f"{max(t_f, t_b) / t_pred:.2f} |", flush=True)
            if a.cross:
                cdev = [(hyper5, X, torch.from_numpy(api.nlml_cross_weights(hyper5, hX, hy)).cuda()) for (_, X, _), (hX, hy) in zip(dev, host)]
                c_pred = timed(api, TIMER_RECON, lambda: api.grid_reconstruct_cross(2, 1, dr, dxs, dps, 2000.0, dx, dp, cdev, None, want_pred=True), a.reps)
                c_sums = timed(api, TIMER_RECON, lambda: api.grid_reconstruct_cross(2, 1, dr, dxs, dps, 2000.0, dx, dp, cdev, None, want_pred=False), a.reps)

                def explicit():
                    for X, y in host:
                        api._check(lib.gple_nlml_cross_predict(api.ctx, _capi._ptr(hyper5), _capi._ptr(X), _capi._ptr(y), N, C.cast(grid_pts.data_ptr(), _capi._dp),
                                                               n * n, _capi.IO_DEVICE, C.cast(mean.data_ptr(), _capi._dp)))
                c_old = float("nan") if a.no_old else timed(api, TIMER_PREDICT, explicit, a.reps)
                b_pred = timed(api, TIMER_RECON, lambda: api.grid_reconstruct(2, 1, dr, dxs, dps, 2000.0, dx, dp, dev, None, want_pred=True), a.reps)
                tiles = lambda g: [(r0, min(r0 + 64, n), min(r0 + 32, n - 1)) for r0 in range(0, n, 64)]
                in_x = np.array([abs(hyper5[2]) * np.abs(x[r0:r1] - x[rc]).max() <= 6.0 for r0, r1, rc in tiles(x)])
                in_p = np.array([abs(hyper5[3]) * np.abs(p[r0:r1] - p[rc]).max() <= 6.0 for r0, r1, rc in tiles(p)])
                cross_rows.append(f"| {n} | {N} | {c_pred:.3f} | {c_sums:.3f} | {np.outer(in_x, in_p).mean():.2f} | {c_old:.2f} | {c_old / c_pred:.1f} | {b_pred:.3f} | "
                                  f"{c_pred / b_pred:.2f} |")
                print("cross " + cross_rows[-1], flush=True)
    if cross_rows:
        print(f"\ncross-term kernel, a = {hyper5[2]:.4g}, c = {hyper5[3]:.4g}, b = {hyper5[4]:.4g}")
        print("| n | N | cross + pred ms | cross ms (sums only) | tiles centred | (a) `gple_nlml_cross_predict` route ms | (a) / cross | (b) `gple_grid_reconstruct` + pred ms | cross / (b) |")
        print("|---|---|---|---|---|---|---|---|---|")
        print("\n".join(cross_rows))
    api.close()


if __name__ == "__main__":
    main()
