"""Time of the ensemble's scatter into a phase-space grid (gple_hop_bin; DESIGN.md §17, "The ensemble in phase space"): GPLE_TIMER_HOP_BIN, the
bin kernel alone, as the median (min - max) over calls after a warm-up call, with hop_observe's wall time on the same ensemble beside it (the
same loads and the same Jacobi solve, a tree sum instead of a scatter; it has no timer of its own, so it is timed around a synchronised call,
launch and read-out included, and hop_bin's wall time taken the same way, clear included, stands next to it as bin_wall_ms).  The ensemble is that of probes/hop_timing.py (DAC at p0 = 16, TSAC at p0 = 10 from the middle surface,
x0 = -4, dt = 1, the bounds far away) after `--steps` steps, at two and three levels, built-in and tabulated at dx = 1 / 16.  Grids over
x in [-8, 8] and p in [-32, 32]: 256 x 256, 961 x 961, and 1 x 1 (every count to one address per surface).  Prints one JSON line.

    python probes/hop_bin_timing.py [--trajectories 1048576] [--steps 250] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gaussian_process_liouville_equation_amd as pkg  # noqa: E402
from gaussian_process_liouville_equation_amd import _capi, pes  # noqa: E402
from tests import hop_numpy as HN  # noqa: E402

MASS, X0, DT, FAR, SEED = 2000.0, -4.0, 1.0, 1e6, 7


def square(n):
    return (-8.0, 16.0 / (n - 1), n, -32.0, 64.0 / (n - 1), n)


GRIDS = {"256x256": square(256), "961x961": square(961), "1x1": (0.0, 1e3, 1, 0.0, 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trajectories", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=250)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    api = pkg.open_api(0)
    api.enable_timing(True)
    rows = []
    try:
        for N, builtin, p0, surface0 in ((2, HN.DAC, 16.0, 0), (3, HN.TSAC, 10.0, 1)):
            t = pes.tabulate(HN.scalar_function(HN.builtin(builtin, N)), -8.0, 1.0 / 16.0, 257)
            user = api.pes_define(N, *t)
            for kind, model in (("built-in", builtin), ("table", user)):
                state = api.hop_sample(N, model, a.trajectories, SEED, X0, p0, 1.0 / (2.0 * p0 / 20.0), p0 / 20.0, surface0, device_out=True)
                state = api.hop_evolve(N, model, state, SEED, MASS, DT, 0, a.steps, -FAR, FAR)
                api.synchronize()
                wall = []
                for k in range(1 + a.reps):  # call 0 warms up
                    t0 = time.perf_counter()
                    sums = api.hop_observe(N, model, state, MASS)
                    wall.append((time.perf_counter() - t0) * 1e3)
                observe = dict(ms=float(np.median(wall[1:])), ms_min=min(wall[1:]), ms_max=max(wall[1:]))
                for label, grid in GRIDS.items():
                    ms = []
                    for k in range(1 + a.reps):
                        acc = api.hop_bin(N, model, state, grid)
                        last, _, _ = api.timing(_capi.TIMER_HOP_BIN)
                        if k:
                            ms.append(last)
                    bin_wall = []  # the whole call as observe's is timed: the clear, the launch and the wait
                    for k in range(1 + a.reps):
                        t0 = time.perf_counter()
                        api.hop_bin(N, model, state, grid)
                        api.synchronize()
                        bin_wall.append((time.perf_counter() - t0) * 1e3)
                    acc = acc.cpu().numpy()
                    n_cells = grid[2] * grid[5]
                    counts = acc[:N * n_cells].reshape(N, n_cells)
                    assert acc[-2] + acc[-1] == a.trajectories
                    if label == "1x1":
                        assert np.array_equal(counts.sum(axis=1), sums[:N])  # everyone runs: observe's counts per surface
                    rows.append(dict(levels=N, model=kind, grid=label, bin_ms=float(np.median(ms)), bin_ms_min=min(ms), bin_ms_max=max(ms),
                                     bin_wall_ms=float(np.median(bin_wall[1:])),
                                     binned=int(acc[-2]), outside=int(acc[-1]), cells_hit=int((counts.sum(axis=0) > 0).sum()), fullest=int(counts.sum(axis=0).max()),
                                     atomics_per_trajectory=1 + N * (N - 1), observe_wall_ms=observe["ms"], observe_wall_ms_min=observe["ms_min"],
                                     observe_wall_ms_max=observe["ms_max"]))
            api.pes_undefine(user)
    finally:
        api.close()
    print(json.dumps(dict(probe="hop_bin_timing", trajectories=a.trajectories, steps=a.steps, reps=a.reps, rows=rows)))


if __name__ == "__main__":
    main()
