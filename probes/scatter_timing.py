"""The march of gple_scatter: GPLE_TIMER_SCATTER of one call, and the wall time of the call, for n_E energies (momenta uniform
in [3, 30] on the lower surface) and N grid steps, on the two-level SAC model and the three-level TSAC model, box [-20, 20], mass 2000.  One
process; per shape a warm-up call, then the median of --reps calls (min - max) on device energies.  A thread is a chain of N + 1 dependent
steps, so the figure that matters is the time of a step: ns per step of a chain, and energy-steps per second over the whole call.

Prints one JSON line.

    python probes/scatter_timing.py [--energies 4096 1048576] [--steps 6000] [--reps 5]
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
from gaussian_process_liouville_equation_amd import _capi  # noqa: E402

MASS, BOX = 2000.0, 20.0
MODELS = (("sac", 2, 0), ("tsac", 3, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--energies", type=int, nargs="+", default=[4096, 1 << 20])
    ap.add_argument("--steps", type=int, default=6000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    api = pkg.open_api(0)
    api.enable_timing(True)
    rows = []
    try:
        import torch

        where = torch.device("cuda", api.device)
        for name, num_pes, model in MODELS:
            lowest = np.linalg.eigvalsh(api.pes_diabatic_n(num_pes, model, [-BOX])[0][0])[0]
            for n_E in a.energies:
                p = np.linspace(3.0, 30.0, n_E)
                energies = torch.from_numpy(p * p / 2.0 / MASS + lowest).to(where)
                kernel, wall = [], []
                for k in range(1 + a.reps):  # call 0 warms up
                    api.synchronize()
                    t0 = time.perf_counter()
                    prob, defect = api.scatter(num_pes, model, MASS, -BOX, BOX, a.steps, energies)
                    seconds = time.perf_counter() - t0
                    if k:
                        kernel.append(api.timing(_capi.TIMER_SCATTER)[0])
                        wall.append(seconds * 1e3)
                worst = float(torch.nan_to_num(defect).abs().max())
                med = float(np.median(kernel))
                rows.append(dict(model=name, num_pes=num_pes, n_energies=n_E, n_steps=a.steps, kernel_ms=dict(median=med, min=min(kernel), max=max(kernel)),
                                 wall_ms=dict(median=float(np.median(wall)), min=min(wall), max=max(wall)), ns_per_chain_step=med * 1e6 / (a.steps + 1),
                                 energy_steps_per_second=n_E * (a.steps + 1) / (med * 1e-3), largest_defect=worst))
    finally:
        api.close()
    print(json.dumps(dict(probe="scatter_timing", reps=a.reps, rows=rows)))


if __name__ == "__main__":
    main()
