"""Fewest-switches surface hopping on Tully's dual avoided crossing at the defaults of the reference's input.py (mass 2000, x0 = -8,
box [-15, 15], sigma_p = p0 / 20): the scattering line of an ensemble of trajectories — head, the fractions that left [left | right][surface],
the fraction still running — and, with a third argument, the DVR flux line of the same model, energy and packet beside it.  The two are
printed for information: surface hopping is a method with an error of its own, and nothing here bounds it.  Run on a GPU box:
    python examples/hopping.py [lnE] [trajectories] [dvr]"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import gaussian_process_liouville_equation_amd as pkg  # noqa: E402
from gaussian_process_liouville_equation_amd import exact, hopping  # noqa: E402

ln_e = float(sys.argv[1]) if len(sys.argv) > 1 else 0.0
n_traj = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
with_dvr = len(sys.argv) > 3
api = pkg.open_api(0)
try:
    res = hopping.run(api, model=hopping.DAC, num_pes=2, ln_energy=ln_e, n_traj=n_traj, seed=1, log=print)
    print(f"{n_traj} trajectories, dt = {res['dt']:g}, {res['steps']} steps in {len(res['records'])} outputs of {res['output_step']} steps; {res['total_seconds']:.2f} s")
    print("FSSH:", res["scattering_line"])
    if with_dvr:
        dvr = exact.run(api, model=exact.DAC, num_pes=2, boundary=exact.ABSORBING, ln_energy=ln_e, write_phase=None, flux=True, until_absorbed=True)
        print("DVR: ", dvr["scattering_line"])
finally:
    api.close()
