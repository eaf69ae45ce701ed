"""Fewest switches, fewest switches with the energy-based decoherence correction, MASH (the mapping approach to surface hopping of Mannouch and
Richardson, J. Chem. Phys. 158, 104111 (2023)) and the exact result of one setup under each other, on Tully's dual avoided crossing at the
defaults of the reference's input.py (mass 2000, x0 = -8, box [-15, 15], sigma_p = p0 / 20).  A line is: head, the fractions that left
[left | right][surface], the fraction still inside.  MASH has an active surface like fewest switches, but it is the adiabatic state with the larger
population, its step draws no random number, and it needs no decoherence correction.  The lines are printed for information; no trajectory method
bounds its own error ("MASH trajectories").  Run on a GPU box:
    python examples/hopping_mash.py [lnE] [trajectories]"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import gaussian_process_liouville_equation_amd as pkg  # noqa: E402
from gaussian_process_liouville_equation_amd import exact, hopping  # noqa: E402

ln_e = float(sys.argv[1]) if len(sys.argv) > 1 else 0.0
n_traj = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
api = pkg.open_api(0)
try:
    lines = {}
    for name, kw in (("FSSH", dict(method="fssh")), ("FSSH+EDC", dict(method="fssh", decoherence="edc")), ("MASH", dict(method="mash"))):
        res = hopping.run(api, model=hopping.DAC, num_pes=2, ln_energy=ln_e, n_traj=n_traj, seed=1, **kw)
        print(f"{name}: {n_traj} trajectories, dt = {res['dt']:g}, {res['steps']} steps; {res['total_seconds']:.2f} s; {res['stop'] or 'ran to the total time'}")
        lines[name] = res["scattering_line"]
    dvr = exact.run(api, model=exact.DAC, num_pes=2, boundary=exact.ABSORBING, ln_energy=ln_e, write_phase=None, flux=True, until_absorbed=True)
    lines["DVR"] = dvr["scattering_line"]
    for name, line in lines.items():
        print(f"{name + ':':<9} {line}")
finally:
    api.close()
