"""Time of the symmetrical quasi-classical step beside the mean-field step it extends (gple_hop_evolve_sqc, gple_hop_evolve_mf; DESIGN.md §17,
"Symmetrical quasi-classical trajectories"): GPLE_TIMER_HOP_SQC and GPLE_TIMER_HOP_MF of one call each, in the same process, the median over
calls after a warm-up call (min - max beside it), at two and three levels, for a built-in model and for the same model tabulated at
dx = 1 / 16.  The yardstick is the mean-field kernel: the SQC force adds NP - 1 additions and one multiply-subtract per evaluation, so at equal
occupancy the ratio is expected near 1.  The protocol is probes/hop_mf_timing.py's: every call starts from a fresh sample (DAC at p0 = 16, TSAC
at p0 = 10 from the middle surface, x0 = -4, dt = 1; the SQC sample on the triangle window at gamma = 1 / 3) with the bounds far away, so all
trajectories run for all the steps of every call.  Prints one JSON line.

    python probes/hop_sqc_timing.py [--trajectories 1048576] [--steps 1000] [--reps 5]
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
WINDOW, GAMMA = _capi.HOP_WINDOW_TRIANGLE, _capi.HOP_WINDOW_GAMMA[_capi.HOP_WINDOW_TRIANGLE]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trajectories", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    api = pkg.open_api(0)
    api.enable_timing(True)
    rows = []
    try:
        for N, builtin, p0, surface0 in ((2, HN.DAC, 16.0, 0), (3, HN.TSAC, 10.0, 1)):
            t = pes.tabulate(HN.scalar_function(HN.builtin(builtin, N)), -8.0, 1.0 / 16.0, 257)
            user = api.pes_define(N, *t)
            sx, sp = 1.0 / (2.0 * p0 / 20.0), p0 / 20.0
            for kind, model in (("built-in", builtin), ("table", user)):
                ms = {"ehrenfest": [], "sqc": []}
                for k in range(1 + a.reps):  # call 0 warms up
                    state = api.hop_sample(N, model, a.trajectories, SEED, X0, p0, sx, sp, surface0, device_out=True)
                    state = api.hop_evolve_mf(N, model, state, MASS, DT, a.steps, -FAR, FAR)
                    mean_field = api.timing(_capi.TIMER_HOP_MF)[0]
                    sums = api.hop_observe_mf(N, model, state, MASS)
                    assert sums[3 * N] == a.trajectories  # every trajectory ran to the end
                    state = api.hop_sample_sqc(N, model, a.trajectories, SEED, X0, p0, sx, sp, surface0, WINDOW, GAMMA, device_out=True)
                    state = api.hop_evolve_sqc(N, model, state, MASS, DT, a.steps, -FAR, FAR, GAMMA)
                    sqc = api.timing(_capi.TIMER_HOP_SQC)[0]
                    sums = api.hop_observe_sqc(N, model, state, MASS, WINDOW, GAMMA)
                    assert sums[3 * N] == a.trajectories
                    if k:
                        ms["ehrenfest"].append(mean_field)
                        ms["sqc"].append(sqc)
                med = {key: float(np.median(v)) for key, v in ms.items()}
                rows.append(dict(levels=N, model=kind, ehrenfest_ms=med["ehrenfest"], ehrenfest_min=min(ms["ehrenfest"]), ehrenfest_max=max(ms["ehrenfest"]),
                                 sqc_ms=med["sqc"], sqc_min=min(ms["sqc"]), sqc_max=max(ms["sqc"]), sqc_over_ehrenfest=med["sqc"] / med["ehrenfest"],
                                 sqc_trajectory_steps_per_second=a.trajectories * a.steps / (med["sqc"] * 1e-3),
                                 ehrenfest_trajectory_steps_per_second=a.trajectories * a.steps / (med["ehrenfest"] * 1e-3),
                                 windowed=(sums[:3 * N].reshape(3, N).sum(axis=0) / a.trajectories).tolist(),
                                 unassigned=float(sums[3 * N + 3:3 * N + 6].sum() / a.trajectories)))
            api.pes_undefine(user)
    finally:
        api.close()
    print(json.dumps(dict(probe="hop_sqc_timing", trajectories=a.trajectories, steps=a.steps, reps=a.reps, rows=rows)))


if __name__ == "__main__":
    main()
