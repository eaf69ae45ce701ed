"""What a change to the potential plumbing costs the built-in models: one N-level tick (gple_evolve_n, wall clock, median of 9
calls after a warm-up; two levels DAC at 1024 points per element, three levels TSAC at 512) and GPLE_TIMER_MQCL per step at n = 961 over calls
of 10 steps, as one JSON line.  ROOT (default: this tree) names the tree whose package is measured, so that a built checkout of another commit
can be measured by the same script; compare medians over several processes per tree, alternating the trees.

    python probes/pes_cost.py [ROOT]
"""
import json
import os
import sys
import time

ROOT = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gaussian_process_liouville_equation_amd as pkg  # noqa: E402
from gaussian_process_liouville_equation_amd import kernels as K  # noqa: E402

assert os.path.abspath(pkg.__file__).startswith(ROOT), pkg.__file__
TH, THC = [1.0, 0.7086, 0.7056, 1e-2], [1.0, 1.1, 0.8, 0.7, 0.9, 0.7, 0.8, 0.05]
TIMER_MQCL = 5


def main():
    api = pkg.open_api(0)
    api.enable_timing(True)
    out = {"root": ROOT}
    for num_pes, model, N in ((2, 1, 1024), (3, 3, 512)):
        rng = np.random.Generator(np.random.PCG64(7 + num_pes))
        dens = {}
        for (i, j) in K.element_order(num_pes):
            r = rng.normal([-0.8, 14.0], [0.7086, 0.7056], size=(N, 2))
            g = np.exp(-0.5 * (((r[:, 0] + 0.8) / 0.7086) ** 2 + ((r[:, 1] - 14.0) / 0.7056) ** 2)) / (2 * np.pi * 0.7086 * 0.7056)
            dens[(i, j)] = (r, (g * ((0.5, 0.3, 0.2)[i] if i == j else 0.15 * np.exp(0.4j * (r[:, 0] + 0.8)))).astype(complex))
        fits = [api.real_fit(TH, *dens[e], 0) if e[0] == e[1] else api.complex_fit(THC, *dens[e], 0) for e in K.element_order(num_pes)]
        api.evolve_n(num_pes, fits, model, 2000.0, 1.0, dens)
        t = []
        for _ in range(9):
            t0 = time.perf_counter()
            api.evolve_n(num_pes, fits, model, 2000.0, 1.0, dens)
            t.append(1e3 * (time.perf_counter() - t0))
        out[f"tick_n{num_pes}_ms"] = float(np.median(t))
        for f in fits:
            f.release()
    n = 961
    i = np.arange(n, dtype=np.float64)
    x = (-15.0 * (n - 1 - i) + 15.0 * i) / (n - 1)
    p = ((63.2 - 50.0) * (n - 1 - i) + (63.2 + 50.0) * i) / (n - 1)
    for num_pes, model in ((2, 1), (3, 3)):  # the state and the arguments of probes/mqcl_timing.py
        rho = np.zeros((num_pes, num_pes, n, n), dtype=np.complex128)
        rho[0, 0] = np.exp(-(((x[:, None] + 8.0) / 0.158) ** 2 + ((p[None, :] - 63.2) / 3.16) ** 2) / 2.0)
        dx_, dp_, r = torch.from_numpy(x).cuda(), torch.from_numpy(p).cuda(), torch.from_numpy(rho).cuda()
        ms = []
        for k in range(8):  # call 0 warms up
            api.mqcl_evolve(num_pes, model, dx_, dp_, r, 2000.0, 30.0, 100.0, 2.0 ** -6, 10)
            if k:
                ms.append(api.timing(TIMER_MQCL)[0])
        out[f"mqcl_961_n{num_pes}_ms_per_step"] = float(np.median(ms)) / 10
    api.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
