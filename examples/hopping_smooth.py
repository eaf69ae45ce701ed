"""The ensemble of examples/hopping_phase.py in phase space twice: once binned (gple_hop_bin / gple_hop_density, every trajectory in its nearest
cell) into out/binned, once smoothed (gple_hop_smooth, a Gaussian kernel density estimate with Scott's bandwidths h = sigma n^(-1/6);
DESIGN.md §17, "The ensemble in phase space, smoothed") into out/smooth.  Both directories hold x.txt, p.txt and phase.txt in the layout of
exact.run, so either lies beside the Wigner function of examples/exact_dvr.py or goes to examples/reconstruct_files.py as it is; the smoothed
field has no counting noise.  Printed per output and run: the population of each state summed from the grid of phase.txt next to the one
hop_observe counts (fewest switches: the running fraction per active surface; with `amplitude`, an Ehrenfest run: the running weights of
hop_observe_mf).  The two differ by what lies off the grid, by the six digits of "%g" and, where a bandwidth is below the grid's spacing, by the
quadrature error 2 exp(-2 pi^2 (h / d)^2) of a sum over the grid (a coarse grid under a narrow packet: take more points).  Run on a GPU box:
    python examples/hopping_smooth.py [lnE] [trajectories] [out] [n_x] [n_p] [amplitude]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import gaussian_process_liouville_equation_amd as pkg  # noqa: E402
from gaussian_process_liouville_equation_amd import hopping, reconstruct  # noqa: E402

ln_e = float(sys.argv[1]) if len(sys.argv) > 1 else 0.0
n_traj = int(sys.argv[2]) if len(sys.argv) > 2 else 1000000
out = sys.argv[3] if len(sys.argv) > 3 else "hopping_smooth_out"
n_x = int(sys.argv[4]) if len(sys.argv) > 4 else 256
n_p = int(sys.argv[5]) if len(sys.argv) > 5 else 256
kind = sys.argv[6] if len(sys.argv) > 6 else None
if kind not in (None, "amplitude"):
    sys.exit("the sixth argument is amplitude, or nothing")
more = {} if kind is None else dict(method="ehrenfest", phase_density="amplitude")
api = pkg.open_api(0)
try:
    for label, smooth in (("binned", None), ("smooth", "scott")):
        where = os.path.join(out, label)
        res = hopping.run(api, model=hopping.DAC, num_pes=2, ln_energy=ln_e, n_traj=n_traj, seed=1, out_dir=where, phase_grid=(n_x, n_p), phase_smooth=smooth, **more)
        x, p = (reconstruct.read_grid(os.path.join(where, name)) for name in ("x.txt", "p.txt"))
        cell = (x[1] - x[0]) * (p[1] - p[0])
        note = "" if smooth is None else f", h = ({res['phase_smooth'][0]:.4g}, {res['phase_smooth'][1]:.4g})"
        print(f"{label}: {n_traj} trajectories on {n_x} x {n_p} points, {len(res['records'])} outputs; {res['total_seconds']:.2f} s; files in {where}{note}")
        print("t  population from the grid of phase.txt | " + ("running fraction per surface of hop_observe" if kind is None else "running weights of hop_observe_mf / n"))
        for rec, block in zip(res["records"], reconstruct.phase_blocks(os.path.join(where, "phase.txt"), 2, n_x, n_p)):
            rho = reconstruct._parse_host(block)[0].view(np.complex128).reshape(2, 2, n_x, n_p)
            grid = [rho[a, a].real.sum() * cell for a in range(2)]
            seen = (rec["counts"] if kind is None else rec["weights"])[hopping.RUNNING] / n_traj
            print(f"{rec['t']:g}  " + " ".join(f"{v:.6f}" for v in grid) + " | " + " ".join(f"{v:.6f}" for v in seen))
finally:
    api.close()
