"""Cost of the absorbing boundary of the MQCLE run (gple_mqcl_evolve_absorbing; DESIGN.md §12, "The absorbing boundary") on the default grid with
its absorber: GPLE_TIMER_MQCL of one call of an output's steps, as the median over calls after a warm-up call (the method of mqcl_timing.py),
beside gple_mqcl_evolve of the same steps on the same grid.

    python probes/mqcl_absorbing_timing.py [--ln-energy 0] [--mask-every 64,40] [--reps 5]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import gaussian_process_liouville_equation_amd as pkg  # noqa: E402
from gaussian_process_liouville_equation_amd import exact, exact_mqcl  # noqa: E402

TIMER_MQCL = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ln-energy", type=float, default=0.0)
    ap.add_argument("--mask-every", default="64,40")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    s = exact_mqcl.setup(a.ln_energy, boundary=exact.ABSORBING)
    n, steps = s["n_grids"], s["output_step"]
    api = pkg.open_api(0)
    api.enable_timing(True)
    print(f"n = {n} ({s['n_absorbing']} absorbing rows a side), {steps} steps per call, dt = {s['dt']:g}; median of {a.reps} calls after a warm-up")
    print("| num_pes | mask_every | absorbing rows | gple_mqcl_evolve ms | gple_mqcl_evolve_absorbing ms | difference |")
    print("|---|---|---|---|---|---|")
    for num_pes in (2, 3):
        model = 1 if num_pes == 2 else 3
        rho = exact_mqcl.initial_density(s["x"], s["p"], s["dx"], s["dp"], s["x0"], s["p0"], s["sigma_x"], s["sigma_p"], num_pes)
        tx, tp = torch.from_numpy(s["x"]).cuda(), torch.from_numpy(s["p"]).cuda()
        r = torch.from_numpy(rho).cuda()
        acc = torch.zeros((2, num_pes, n), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()

        def median(call):
            ms = []
            for k in range(1 + a.reps):  # call 0 warms up
                call()
                api.synchronize()
                if k:
                    ms.append(api.timing(TIMER_MQCL)[0])
            return float(np.median(ms))

        plain = median(lambda: api.mqcl_evolve(num_pes, model, tx, tp, r, s["mass"], s["length_x"], s["length_p"], s["dt"], steps))
        for mask_every in [int(v) for v in a.mask_every.split(",")]:
            g = exact_mqcl.half_mask(s["x"], s["mass"], s["xmin"], s["xmax"], s["absorbing_length"], mask_every * s["dt"])
            tg = torch.from_numpy(g).cuda()
            torch.cuda.synchronize()
            masked = median(lambda: api.mqcl_evolve_absorbing(num_pes, model, tx, tp, r, s["mass"], s["length_x"], s["length_p"], s["dt"], steps, mask_every,
                                                              tg, s["n_left"], acc))
            print(f"| {num_pes} | {mask_every} | {int((g != 0).sum())} | {plain:.1f} | {masked:.1f} | {100.0 * (masked - plain) / plain:+.2f} % |", flush=True)
    api.close()


if __name__ == "__main__":
    main()
