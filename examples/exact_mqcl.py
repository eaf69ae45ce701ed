"""Exact MQCLE phase-space dynamics of Tully's dual avoided crossing at the defaults of the reference's input.py (mass 2000, x0 = -8,
box [-15, 15], sigma_p = p0 / 20, about 50 outputs), as liouville_equation/main.cpp runs it: the five files x.txt, p.txt, t.txt, phase.txt
and averages.txt in an output directory and the final stdout line.  Run on a GPU box:
    python examples/exact_mqcl.py [lnE] [out_dir] [text|npy|none]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import gaussian_process_liouville_equation_amd as pkg  # noqa: E402
from gaussian_process_liouville_equation_amd import exact_mqcl  # noqa: E402

ln_e = float(sys.argv[1]) if len(sys.argv) > 1 else 0.0
out_dir = sys.argv[2] if len(sys.argv) > 2 else "exact_mqcl_out"
write_phase = sys.argv[3] if len(sys.argv) > 3 else "text"
api = pkg.open_api(0)
try:
    res = exact_mqcl.run(api, model=exact_mqcl.DAC, num_pes=2, ln_energy=ln_e, out_dir=out_dir,
                         write_phase=None if write_phase == "none" else write_phase, log=print)
    s = res["setup"]
    print(f"grid: {s['n_grids']} x {s['n_grids']}, dx = {s['dx']:g}, dt = {s['dt']:g}; {len(res['records'])} outputs, "
          f"{res['seconds_per_output']:.2f} s per output ({s['output_step']} steps); total {res['total_seconds']:.1f} s")
    print("final populations:", np.array2string(res["records"][-1]["populations"], precision=6))
    print(res["final_line"])
finally:
    api.close()
