"""Exact MQCLE phase-space dynamics of Tully's dual avoided crossing at the defaults of the reference's input.py (mass 2000, x0 = -8,
box [-15, 15], sigma_p = p0 / 20, about 50 outputs), as liouville_equation/main.cpp runs it: the five files x.txt, p.txt, t.txt, phase.txt
and averages.txt in an output directory and the final stdout line.  Run on a GPU box:
    python examples/exact_mqcl.py [lnE] [out_dir] [text|npy|none] [absorbing [flux]]
absorbing: the box grows by the absorber and every block of steps runs between two half-masks ("The absorbing boundary"):
absorbed.txt, absorbed_p.txt and the scattering line beside the other files.  flux: the run goes on until the packet has left, and the DVR
flux line and a 100000-trajectory FSSH line are printed under the MQCLE's."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import gaussian_process_liouville_equation_amd as pkg  # noqa: E402
from gaussian_process_liouville_equation_amd import exact, exact_mqcl, hopping  # noqa: E402

ln_e = float(sys.argv[1]) if len(sys.argv) > 1 else 0.0
out_dir = sys.argv[2] if len(sys.argv) > 2 else "exact_mqcl_out"
write_phase = sys.argv[3] if len(sys.argv) > 3 else "text"
absorbing = len(sys.argv) > 4 and sys.argv[4] == "absorbing"
flux = absorbing and len(sys.argv) > 5 and sys.argv[5] == "flux"
api = pkg.open_api(0)
try:
    kw = dict(boundary=exact.ABSORBING, until_absorbed=flux) if absorbing else {}
    res = exact_mqcl.run(api, model=exact_mqcl.DAC, num_pes=2, ln_energy=ln_e, out_dir=out_dir,
                         write_phase=None if write_phase == "none" else write_phase, log=print, **kw)
    s = res["setup"]
    print(f"grid: {s['n_grids']} x {s['n_grids']}, dx = {s['dx']:g}, dt = {s['dt']:g}; {len(res['records'])} outputs, "
          f"{res['seconds_per_output']:.2f} s per output ({s['output_step']} steps); total {res['total_seconds']:.1f} s")
    print("final populations:", np.array2string(res["records"][-1]["populations"], precision=6))
    print(res["final_line"])
    if absorbing:
        print("MQCLE:", res["scattering_line"])
    if flux:
        dvr = exact.run(api, model=exact.DAC, num_pes=2, boundary=exact.ABSORBING, ln_energy=ln_e, write_phase=None, flux=True, until_absorbed=True)
        print("DVR:  ", dvr["scattering_line"])
        hop = hopping.run(api, model=hopping.DAC, num_pes=2, ln_energy=ln_e, n_traj=100000, seed=1)
        print("FSSH: ", hop["scattering_line"])
finally:
    api.close()
