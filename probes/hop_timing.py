"""Throughput of the surface hopping step (gple_hop_evolve): trajectory-steps per second from GPLE_TIMER_HOP, the median over
calls after a warm-up call, at two and three levels, for a built-in model and for the same model tabulated at dx = 1 / 16.  Every call starts
from a fresh sample of the same ensemble (DAC at p0 = 16, TSAC at p0 = 10 from the middle surface, x0 = -4, dt = 1) with the bounds far away,
so all trajectories run for all the steps of every call and cross the coupling region.  The numpy restatement's seconds per step on the same
box go beside it as the test helper's baseline (not a result).  Prints one JSON line.

    python probes/hop_timing.py [--trajectories 1048576] [--steps 1000] [--reps 5] [--numpy-trajectories 293]
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
from gaussian_process_liouville_equation_amd import pes  # noqa: E402
from tests import hop_numpy as HN  # noqa: E402

TIMER_HOP = 12
MASS, X0, DT, FAR, SEED = 2000.0, -4.0, 1.0, 1e6, 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trajectories", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--numpy-trajectories", type=int, default=293)
    a = ap.parse_args()
    api = pkg.open_api(0)
    api.enable_timing(True)
    rows = []
    try:
        for N, builtin, p0, surface0 in ((2, HN.DAC, 16.0, 0), (3, HN.TSAC, 10.0, 1)):
            potential = HN.builtin(builtin, N)
            t = pes.tabulate(HN.scalar_function(potential), -8.0, 1.0 / 16.0, 257)
            user = api.pes_define(N, *t)
            sx, sp = 1.0 / (2.0 * p0 / 20.0), p0 / 20.0
            for kind, model in (("built-in", builtin), ("table", user)):
                ms = []
                for k in range(1 + a.reps):  # call 0 warms up
                    state = api.hop_sample(N, model, a.trajectories, SEED, X0, p0, sx, sp, surface0, device_out=True)
                    state = api.hop_evolve(N, model, state, SEED, MASS, DT, 0, a.steps, -FAR, FAR)
                    last, _, _ = api.timing(TIMER_HOP)
                    if k:
                        ms.append(last)
                sums = api.hop_observe(N, model, state, MASS)
                assert sums[:N].sum() == a.trajectories  # every trajectory ran to the end
                med = float(np.median(ms))
                rows.append(dict(levels=N, model=kind, ms_per_call=med, ms_min=min(ms), ms_max=max(ms),
                                 trajectory_steps_per_second=a.trajectories * a.steps / (med * 1e-3)))
            api.pes_undefine(user)
            start = HN.sample(potential, N, a.numpy_trajectories, SEED, X0, p0, sx, sp, surface0)
            t0 = time.perf_counter()
            HN.evolve(potential, start, SEED, MASS, DT, 0, 50, -FAR, FAR)
            rows.append(dict(levels=N, model="numpy restatement (baseline)", trajectories=a.numpy_trajectories, seconds_per_step=(time.perf_counter() - t0) / 50))
    finally:
        api.close()
    print(json.dumps(dict(probe="hop_timing", trajectories=a.trajectories, steps=a.steps, reps=a.reps, rows=rows)))


if __name__ == "__main__":
    main()
