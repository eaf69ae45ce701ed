"""What leaves the box, resolved: one trajectory ensemble on Tully's dual avoided crossing binned by its outgoing momentum and by the energy its
method conserves, per side and adiabatic level (hopping.run(outgoing=...), gple_hop_outgoing; DESIGN.md §17, "What left the box"), beside the
two exact solvers on grids that line up with theirs.  Run on a GPU box:
    python examples/hopping_outgoing.py [lnE] [n_traj] [out_dir] [fssh|ehrenfest|sqc|mash]
The momentum grid is the p grid of the absorbing MQCLE run of the same setup, so out_dir/outgoing_p.txt lines up with out_dir/mqcl/absorbed_p.txt
column for column; the centres of the energy grid are the energies of the absorbing DVR run's spectrum, so out_dir/outgoing_e.txt lines up
with out_dir/dvr/spectrum.txt line for line.  Per channel the population and the mean outgoing momentum of the three solvers are printed under
each other (the DVR resolves energy, not momentum: its mean is that of sqrt(2 m (E - E_k)) at the asymptote of level k).  Nothing is asserted."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import gaussian_process_liouville_equation_amd as pkg  # noqa: E402
from gaussian_process_liouville_equation_amd import exact, exact_mqcl, hopping  # noqa: E402

ln_e = float(sys.argv[1]) if len(sys.argv) > 1 else 0.0
n_traj = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
out_dir = sys.argv[3] if len(sys.argv) > 3 else "hopping_outgoing_out"
method = sys.argv[4] if len(sys.argv) > 4 else "fssh"
N_E = 64


def moments(density, q, step):
    """per channel (2, num_pes): the population sum density step, and the mean of q over it (nan where nothing left)"""
    population = density.sum(axis=2) * step
    with np.errstate(invalid="ignore", divide="ignore"):
        return population, (density * q).sum(axis=2) * step / population


def show(label, population, mean):
    for side, name in enumerate(("left ", "right")):
        print(f"{label} {name}:", " ".join(f"level {k}: {population[side, k]:.5f} <p> = {mean[side, k]:8.4f}" for k in range(population.shape[1])))


api = pkg.open_api(0)
try:
    mqcl = exact_mqcl.run(api, model=exact_mqcl.DAC, num_pes=2, ln_energy=ln_e, out_dir=os.path.join(out_dir, "mqcl"), write_phase=None,
                          boundary=exact.ABSORBING, until_absorbed=True)
    s = mqcl["setup"]
    p_grid = (float(s["p"][0]), float(s["dp"]), int(s["n_grids"]))
    # the default energy grid of this setup: p0 -+ 3 sigma_p on the start surface
    e_grid = hopping.outgoing_grids(api, 2, hopping.DAC, exact.setup(ln_e, boundary=exact.ABSORBING), 0, {"energy": N_E})["energy"]
    centres = e_grid[0] + e_grid[1] * np.arange(e_grid[2])
    dvr = exact.run(api, model=exact.DAC, num_pes=2, boundary=exact.ABSORBING, ln_energy=ln_e, write_phase=None, out_dir=os.path.join(out_dir, "dvr"),
                    flux=True, until_absorbed=True, spectrum=centres)
    hop = hopping.run(api, model=hopping.DAC, num_pes=2, ln_energy=ln_e, n_traj=n_traj, seed=1, method=method, out_dir=out_dir,
                      outgoing={"momentum": p_grid, "energy": e_grid}, log=print)
    print("MQCLE:", mqcl["scattering_line"])
    print("DVR:  ", dvr["scattering_line"])
    print(f"{method}:", hop["scattering_line"])
    for axis in ("momentum", "energy"):
        print(axis, "tallies:", hop["outgoing"][axis]["tallies"])
    p = p_grid[0] + p_grid[1] * np.arange(p_grid[2])
    show("MQCLE", *moments(np.asarray(mqcl["absorbed_p"]).reshape(2, 2, -1), p, p_grid[1]))
    show(f"{method:5s}", *moments(hop["outgoing"]["momentum"]["density"], p, p_grid[1]))
    E_far = np.asarray(api.pes_adiabatic_n(2, exact.DAC, np.array([s["xmin"], s["xmax"]]))[0])  # the asymptotes, [side][level]
    spectrum = np.asarray(dvr["spectrum"])[:, 1:].T.reshape(2, 2, -1)
    with np.errstate(invalid="ignore"):
        p_of_E = np.sqrt(2.0 * s["mass"] * (centres[None, None, :] - E_far[:, :, None])) * np.array([-1.0, 1.0])[:, None, None]
    p_of_E = np.where(np.isfinite(p_of_E), p_of_E, 0.0)
    population, _ = moments(spectrum, centres, e_grid[1])
    with np.errstate(invalid="ignore", divide="ignore"):
        show("DVR  ", population, (spectrum * p_of_E).sum(axis=2) * e_grid[1] / population)
    print(f"files: {out_dir}/outgoing_p.txt beside {out_dir}/mqcl/absorbed_p.txt, {out_dir}/outgoing_e.txt beside {out_dir}/dvr/spectrum.txt")
finally:
    api.close()
