"""The fewest-switches ensemble of examples/hopping.py where the MQCLE and the GP live, in phase space: the run also bins its running
trajectories into an n_x x n_p grid at every output time (gple_hop_bin / gple_hop_density) and writes x.txt, p.txt and phase.txt,
the adiabatic density matrix in the layout of exact.run and exact_mqcl.run.  Printed per output: the fraction binned, and the population of
each surface from the grid next to the fraction of running trajectories hop_observe counts on it.  The raw histogram is noisy; the GP fit of
examples/reconstruct_files.py out recon 200 is the smoother, and reads the directory as it is.  The sixth argument picks the ensemble and the
prescription: fssh (the default, the above), fssh-amplitude (the same trajectories with the populations taken from the amplitudes too,
gple_hop_bin_mf / gple_hop_density_mf) or ehrenfest (mean-field trajectories, whose density the amplitudes define); for these two the table
holds binned_weights / n next to the populations hop_observe / hop_observe_mf sum over the running trajectories.  Run on a GPU box:
    python examples/hopping_phase.py [lnE] [trajectories] [out] [n_x] [n_p] [fssh | fssh-amplitude | ehrenfest]"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import gaussian_process_liouville_equation_amd as pkg  # noqa: E402
from gaussian_process_liouville_equation_amd import hopping  # noqa: E402

ln_e = float(sys.argv[1]) if len(sys.argv) > 1 else 0.0
n_traj = int(sys.argv[2]) if len(sys.argv) > 2 else 1000000
out = sys.argv[3] if len(sys.argv) > 3 else "hopping_phase_out"
n_x = int(sys.argv[4]) if len(sys.argv) > 4 else 256
n_p = int(sys.argv[5]) if len(sys.argv) > 5 else 256
kind = sys.argv[6] if len(sys.argv) > 6 else "fssh"
if kind not in ("fssh", "fssh-amplitude", "ehrenfest"):
    sys.exit("the sixth argument is fssh, fssh-amplitude or ehrenfest")
more = {} if kind == "fssh" else dict(method=kind.split("-")[0], phase_density="amplitude")
api = pkg.open_api(0)
try:
    res = hopping.run(api, model=hopping.DAC, num_pes=2, ln_energy=ln_e, n_traj=n_traj, seed=1, out_dir=out, phase_grid=(n_x, n_p), log=print, **more)
    print(f"{n_traj} trajectories on {n_x} x {n_p} points, {len(res['records'])} outputs of {res['output_step']} steps; {res['total_seconds']:.2f} s; files in {out}")
    if kind == "fssh":
        print("t  binned  outside  population from the grid | running fraction of hop_observe, per surface")
    else:
        print("t  binned  outside  population from the grid (binned_weights / n) | " +
              ("running weights of hop_observe_mf / n" if kind == "ehrenfest" else "mean |c_k|^2 of hop_observe over ALL trajectories") + ", per state")
    for rec in res["records"]:
        if kind == "fssh":
            grid, seen = rec["binned_counts"] / n_traj, rec["counts"][hopping.RUNNING] / n_traj
        else:
            grid, seen = rec["binned_weights"] / n_traj, (rec["weights"][hopping.RUNNING] / n_traj if kind == "ehrenfest" else rec["populations"])
        print(f"{rec['t']:g}  {rec['binned'] / n_traj:.6f}  {rec['outside'] / n_traj:.6f}  " + " ".join(f"{v:.6f}" for v in grid) + " | " + " ".join(f"{v:.6f}" for v in seen))
    print("Ehrenfest:" if kind == "ehrenfest" else "FSSH:", res["scattering_line"])
finally:
    api.close()
