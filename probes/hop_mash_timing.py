"""Time of the MASH step beside the fewest-switches step it is a subset of (gple_hop_evolve_mash, gple_hop_evolve; DESIGN.md §17, "MASH
trajectories"): GPLE_TIMER_HOP_MASH and GPLE_TIMER_HOP of one call each, in the same process, the median over calls after a warm-up call
(min - max beside it), for the built-in dual avoided crossing and for the same model tabulated at dx = 1 / 16.  The yardstick is the
fewest-switches kernel of the same run: the MASH step is that step without the hop probabilities and the random number, one comparison in their
place, so its median is expected not to exceed the other's by more than the other's own min - max spread.  The ensemble is
probes/hop_timing.py's: every call starts from a fresh sample (DAC at p0 = 16, x0 = -4, dt = 1) with the bounds far away, so all trajectories
run for all the steps of every call.  Prints one JSON line.

    python probes/hop_mash_timing.py [--trajectories 1048576] [--steps 1000] [--reps 5]
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

TIMER_HOP = 12
MASS, X0, P0, DT, FAR, SEED = 2000.0, -4.0, 16.0, 1.0, 1e6, 7


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
        t = pes.tabulate(HN.scalar_function(HN.builtin(HN.DAC, 2)), -8.0, 1.0 / 16.0, 257)
        user = api.pes_define(2, *t)
        sx, sp = 1.0 / (2.0 * P0 / 20.0), P0 / 20.0
        for kind, model in (("built-in", HN.DAC), ("table", user)):
            ms = {"fssh": [], "mash": []}
            for k in range(1 + a.reps):  # call 0 warms up
                state = api.hop_sample(2, model, a.trajectories, SEED, X0, P0, sx, sp, 0, device_out=True)
                state = api.hop_evolve(2, model, state, SEED, MASS, DT, 0, a.steps, -FAR, FAR)
                fssh = api.timing(TIMER_HOP)[0]
                sums = api.hop_observe(2, model, state, MASS)
                assert sums[:2].sum() == a.trajectories  # every trajectory ran to the end
                state = api.hop_sample_mash(2, model, a.trajectories, SEED, X0, P0, sx, sp, 0, device_out=True)
                state = api.hop_evolve_mash(2, model, state, MASS, DT, a.steps, -FAR, FAR)
                mash = api.timing(_capi.TIMER_HOP_MASH)[0]
                sums = api.hop_observe(2, model, state, MASS)
                assert sums[:2].sum() == a.trajectories
                if k:
                    ms["fssh"].append(fssh)
                    ms["mash"].append(mash)
            med = {key: float(np.median(v)) for key, v in ms.items()}
            rows.append(dict(model=kind, fssh_ms=med["fssh"], fssh_min=min(ms["fssh"]), fssh_max=max(ms["fssh"]), mash_ms=med["mash"], mash_min=min(ms["mash"]),
                             mash_max=max(ms["mash"]), mash_over_fssh=med["mash"] / med["fssh"], excess_ms=med["mash"] - med["fssh"],
                             fssh_spread_ms=max(ms["fssh"]) - min(ms["fssh"]), mash_trajectory_steps_per_second=a.trajectories * a.steps / (med["mash"] * 1e-3),
                             fssh_trajectory_steps_per_second=a.trajectories * a.steps / (med["fssh"] * 1e-3),
                             mash_active_surface=(sums[:2] / a.trajectories).tolist()))
        api.pes_undefine(user)
    finally:
        api.close()
    print(json.dumps(dict(probe="hop_mash_timing", trajectories=a.trajectories, steps=a.steps, reps=a.reps, rows=rows)))


if __name__ == "__main__":
    main()
