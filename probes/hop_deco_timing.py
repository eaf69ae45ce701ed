"""What the decoherence correction of the surface hopping step costs (gple_hop_evolve_dc, step 6a; DESIGN.md §17, "Decoherence corrections"):
GPLE_TIMER_HOP of one call per mode, the median over calls after a warm-up call (min - max beside it), at two and three levels, for a built-in
model and for the same model tabulated at dx = 1 / 16, all in one process.  The yardstick is the row of mode "none" of the same process: that
is gple_hop_evolve's own kernel.  The ensembles are probes/hop_timing.py's: every call starts from a fresh sample (DAC at p0 = 16, TSAC at
p0 = 10 from the middle surface, x0 = -4, dt = 1) with the bounds far away, so all trajectories run for all the steps of every call.  Prints
one JSON line.

    python probes/hop_deco_timing.py [--trajectories 1048576] [--steps 1000] [--reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gaussian_process_liouville_equation_amd as pkg  # noqa: E402
from gaussian_process_liouville_equation_amd import pes  # noqa: E402
from tests import hop_numpy as HN  # noqa: E402

TIMER_HOP = 12
MASS, X0, DT, FAR, SEED, EDC_C = 2000.0, -4.0, 1.0, 1e6, 7, 0.1
MODES = ("none", "edc", "collapse_hop", "collapse_attempt")


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
                base = None
                for mode in MODES:
                    ms = []
                    for k in range(1 + a.reps):  # call 0 warms up
                        state = api.hop_sample(N, model, a.trajectories, SEED, X0, p0, sx, sp, surface0, device_out=True)
                        state = api.hop_evolve(N, model, state, SEED, MASS, DT, 0, a.steps, -FAR, FAR, decoherence=mode, edc_c=EDC_C)
                        last, _, _ = api.timing(TIMER_HOP)
                        if k:
                            ms.append(last)
                    sums = api.hop_observe(N, model, state, MASS)
                    assert sums[:N].sum() == a.trajectories  # every trajectory ran to the end
                    med = float(np.median(ms))
                    base = med if mode == "none" else base
                    rows.append(dict(levels=N, model=kind, mode=mode, ms_per_call=med, ms_min=min(ms), ms_max=max(ms), over_none=med / base,
                                     trajectory_steps_per_second=a.trajectories * a.steps / (med * 1e-3), mean_populations=(sums[3 * N:4 * N] / a.trajectories).tolist(),
                                     fraction_on_surface=(sums[:N] / a.trajectories).tolist()))
            api.pes_undefine(user)
    finally:
        api.close()
    print(json.dumps(dict(probe="hop_deco_timing", trajectories=a.trajectories, steps=a.steps, reps=a.reps, edc_c=EDC_C, rows=rows)))


if __name__ == "__main__":
    main()
