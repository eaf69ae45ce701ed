"""The reference's reconstruction experiment (test/main_evolve.cpp) on the exact MQCLE dynamics of Tully's dual avoided crossing: at every
output time the adiabatic phase-space density is surveyed, n_points points per density-matrix element are drawn weighted by |rho|, the NLML GP
is fitted, predicted back on the whole grid and compared with the exact density, before and after the population / energy constraints.
Writes x.txt, p.txt, t.txt, averages.txt, log.txt and choose.txt.  A trailing `cross` fits the reference's default kernel, the ARD weight
matrix with its cross term (five hyper-parameters per plane), instead of the NOCROSS build's diagonal one; a trailing `batched` (after it)
searches the hyper-parameters of all planes in lock-step on the batched NLML kernel (fit="batched").  Run on a GPU box:
    python examples/reconstruct.py [lnE] [out_dir] [n_points] [max_outputs] [cross] [batched]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import gaussian_process_liouville_equation_amd as pkg  # noqa: E402
from gaussian_process_liouville_equation_amd import reconstruct  # noqa: E402

argv = sys.argv[1:]
kernel, fit = "nocross", "serial"
if argv and argv[-1] == "batched":
    fit, argv = "batched", argv[:-1]
if argv and argv[-1] == "cross":
    kernel, argv = "cross", argv[:-1]
ln_e = float(argv[0]) if len(argv) > 0 else 0.0
out_dir = argv[1] if len(argv) > 1 else "reconstruct_out"
n_points = int(argv[2]) if len(argv) > 2 else 200
max_outputs = int(argv[3]) if len(argv) > 3 else None
api = pkg.open_api(0)
try:
    res = reconstruct.run_mqcl(api, out_dir=out_dir, ln_energy=ln_e, n_points=n_points, seed=20240607, max_outputs=max_outputs, log=print, kernel=kernel, fit=fit)
    recs = res["reconstructions"]
    phases = {k: float(np.mean([r["seconds"][k] for r in recs])) for k in recs[0]["seconds"]}
    print(f"{len(recs)} output times; per output: MQCLE steps {res['seconds_per_output'] - sum(phases.values()):.3f} s, "
          + ", ".join(f"{k} {1e3 * v:.1f} ms" for k, v in phases.items()))
    last = recs[-1]
    print(f"last output: {int((~last['is_small']).sum())} planes fitted, {last['evaluations']} NLML evaluations, MSE {np.array2string(last['mse_after'], precision=3)}")
    print(res["final_line"])
finally:
    api.close()
