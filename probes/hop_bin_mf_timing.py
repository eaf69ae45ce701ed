"""Time of the scatter of an ensemble's amplitudes into a phase-space grid (gple_hop_bin_mf; DESIGN.md §17, "The ensemble in phase space, from the
amplitudes") beside the scatter it extends (gple_hop_bin), in one process: GPLE_TIMER_HOP_BIN_MF and GPLE_TIMER_HOP_BIN, each the bin kernel
alone, as the median (min - max) over calls after a warm-up call, taken in turn on the same state and grid.  The yardstick is hop_bin's kernel
scaled by the ratio of atomic adds per trajectory, num_pes^2 against 1 + num_pes (num_pes - 1): 4 / 3 at two levels, 9 / 7 at three.  The
ensemble is that of probes/hop_bin_timing.py (DAC at p0 = 16, TSAC at p0 = 10 from the middle surface, x0 = -4, dt = 1, the bounds far away,
`--steps` fewest-switches steps), at two and three levels, built-in and tabulated at dx = 1 / 16; grids over x in [-8, 8] and p in [-32, 32],
256 x 256 and 961 x 961.  Prints one JSON line.

    python probes/hop_bin_mf_timing.py [--trajectories 1048576] [--steps 250] [--reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gaussian_process_liouville_equation_amd as pkg  # noqa: E402
from gaussian_process_liouville_equation_amd import _capi, pes  # noqa: E402
from tests import hop_numpy as HN  # noqa: E402

MASS, X0, DT, FAR, SEED = 2000.0, -4.0, 1.0, 1e6, 7


def square(n):
    return (-8.0, 16.0 / (n - 1), n, -32.0, 64.0 / (n - 1), n)


GRIDS = {"256x256": square(256), "961x961": square(961)}


def spread(ms):
    return dict(ms=float(np.median(ms)), ms_min=min(ms), ms_max=max(ms))


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
                for label, grid in GRIDS.items():
                    mixed_ms, mf_ms = [], []
                    for k in range(1 + a.reps):  # call 0 of either warms up; the two take turns
                        mixed = api.hop_bin(N, model, state, grid)
                        last = api.timing(_capi.TIMER_HOP_BIN)[0]
                        mf = api.hop_bin_mf(N, model, state, grid)
                        last_mf = api.timing(_capi.TIMER_HOP_BIN_MF)[0]
                        if k:
                            mixed_ms.append(last)
                            mf_ms.append(last_mf)
                    mixed, mf = mixed.cpu().numpy(), mf.cpu().numpy()
                    n_cells = grid[2] * grid[5]
                    count = mixed[:N * n_cells].reshape(N, n_cells).sum(axis=0)
                    off = np.abs(mf[:N * n_cells].reshape(N, n_cells).sum(axis=0) - 4294967296 * count)
                    assert np.array_equal(mf[-2:], mixed[-2:]) and mf[-2] + mf[-1] == a.trajectories and (off <= count * (N / 2.0 + 1.0)).all()
                    adds = N * N / (1.0 + N * (N - 1))
                    one, two = spread(mixed_ms), spread(mf_ms)
                    rows.append(dict(levels=N, model=kind, grid=label, bin_ms=one["ms"], bin_ms_min=one["ms_min"], bin_ms_max=one["ms_max"],
                                     bin_mf_ms=two["ms"], bin_mf_ms_min=two["ms_min"], bin_mf_ms_max=two["ms_max"], ratio=two["ms"] / one["ms"],
                                     adds_ratio=adds, ratio_to_scaled=two["ms"] / (adds * one["ms"]), bin_spread=one["ms_max"] / one["ms_min"],
                                     binned=int(mf[-2]), outside=int(mf[-1]), cells_hit=int((count > 0).sum()), fullest=int(count.max()),
                                     worst_cell_sum_off=int(off.max())))
            api.pes_undefine(user)
    finally:
        api.close()
    print(json.dumps(dict(probe="hop_bin_mf_timing", trajectories=a.trajectories, steps=a.steps, reps=a.reps, rows=rows)))


if __name__ == "__main__":
    main()
