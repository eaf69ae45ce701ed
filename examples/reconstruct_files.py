"""The reference's reconstruction experiment (test/main_evolve.cpp, test/main_screenshot.cpp) on a directory that one of the exact solvers
wrote — `python examples/exact_mqcl.py 0 out text`, `python examples/exact_dvr.py 0 out text`, or the reference's own programs: x.txt, p.txt,
t.txt and phase.txt are read back, every output time of phase.txt is converted to doubles on the device (gple_parse_g) and reconstructed there.
Writes log.txt and choose.txt into out_dir (default: in_dir).  index: one output time alone (main_screenshot.cpp) or `all`; a trailing `cross`
fits the cross-term kernel, a trailing `batched` (after it) searches all planes in lock-step.  Run on a GPU box:
    python examples/reconstruct_files.py in_dir [out_dir] [n_points] [index] [cross] [batched]"""
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
if not argv:
    sys.exit(__doc__)
in_dir = argv[0]
out_dir = argv[1] if len(argv) > 1 else in_dir
n_points = int(argv[2]) if len(argv) > 2 else 200
outputs = [int(argv[3])] if len(argv) > 3 and argv[3] != "all" else None
api = pkg.open_api(0)
try:
    recs = reconstruct.run_files(api, in_dir, out_dir=out_dir, n_points=n_points, seed=20240607, outputs=outputs, log=print, kernel=kernel, fit=fit)
    phases = {k: float(np.mean([r["seconds"][k] for r in recs])) for k in recs[0]["seconds"]}
    print(f"{len(recs)} output times; per output: " + ", ".join(f"{k} {1e3 * v:.1f} ms" for k, v in phases.items()))
    last = recs[-1]
    print(f"last output: {int((~last['is_small']).sum())} planes fitted, {last['evaluations']} NLML evaluations, MSE {np.array2string(last['mse_after'], precision=3)}")
finally:
    api.close()
