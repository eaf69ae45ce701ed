"""Tully's plot on the dual avoided crossing: the branching probabilities as a function of the incoming momentum, from ONE grouped ensemble of
surface hopping trajectories (hopping.scan; DESIGN.md §17, "A curve in one launch") beside the energy-resolved channels of ONE absorbing DVR
run (exact.run(spectrum=n_E)).  The momenta are the n_E the spectrum uses by default, uniform over p0 +- 3 sigma_p of the packet
at ln E; every trajectory of a momentum starts at x0 with exactly that momentum (Tully's convention, which is what an energy-resolved exact
curve is to be compared with).  Per momentum: p, then the hopping fractions [left | right][surface] with the largest of their standard errors,
then the DVR fractions of the same channels.  The two are printed for information: surface hopping is a method with an error of its own, and
nothing here bounds it.  Run on a GPU box:
    python examples/hopping_scan.py [lnE] [n_per_group] [n_E]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import gaussian_process_liouville_equation_amd as pkg  # noqa: E402
from gaussian_process_liouville_equation_amd import exact, hopping  # noqa: E402

ln_e = float(sys.argv[1]) if len(sys.argv) > 1 else 0.0
n_per_group = int(sys.argv[2]) if len(sys.argv) > 2 else 16384
n_E = int(sys.argv[3]) if len(sys.argv) > 3 else 64
s = exact.setup(ln_e, boundary=exact.ABSORBING)
momenta = np.linspace(s["p0"] - 3.0 * s["sigma_p"], s["p0"] + 3.0 * s["sigma_p"], n_E) if n_E > 1 else np.array([s["p0"]])  # exact.spectrum_energies
api = pkg.open_api(0)
try:
    res = hopping.scan(api, model=hopping.DAC, num_pes=2, momenta=momenta, n_per_group=n_per_group, seed=1, fixed=True, log=print)
    print(f"FSSH: {n_E} momenta x {n_per_group} trajectories, dt = {res['dt'].min():g} ... {res['dt'].max():g}, {res['steps']} steps in launches of 4096; "
          f"{res['total_seconds']:.2f} s")
    dvr = exact.run(api, model=exact.DAC, num_pes=2, boundary=exact.ABSORBING, ln_energy=ln_e, write_phase=None, flux=True, until_absorbed=True, spectrum=n_E)
    print(f"DVR:  spectrum of {n_E} energies over 2^{dvr['spectrum_levels']} steps, {dvr['total_seconds'] + dvr['spectrum_seconds']:.2f} s")
    rho = dvr["spectrum"][:, 1:]
    held = rho.sum(axis=1) > 1e-3 * rho.sum(axis=1).max()  # energies the packet hardly holds have no DVR figure
    print("p | FSSH left 0, left 1, right 0, right 1 (+- largest standard error) | DVR the same channels")
    for g in range(n_E):
        fssh = " ".join(exact.fmt(v) for v in res["scattered"][g].reshape(-1))
        exact_part = " ".join(exact.fmt(v) for v in rho[g] / rho[g].sum()) if held[g] else "-"
        print(f"{exact.fmt(momenta[g])} | {fssh} (+- {exact.fmt(res['stderr'][g].max())}) | {exact_part}")
finally:
    api.close()
