"""Overcoherence where it shows: extended coupling with reflection (ECR) entered on the UPPER adiabatic surface at p0 = 10, which reflects the
packet back through the coupling region.  hopping.scan runs the same grouped ensemble twice, as Tully's algorithm stands and with the
energy-based decoherence correction (decoherence="edc"; DESIGN.md §17, "Decoherence corrections"), and each momentum is printed beside the
energy-resolved channels of ONE absorbing DVR run of the same packet (exact.run(spectrum=...)), as examples/hopping_scan.py does.
The DVR packet is put on the upper surface here (exact.run itself starts on the lowest one) and its energies are p^2 / 2m above the upper surface
at x0.  The momenta are n_momenta values uniform over p0 +- 3 sigma_p; every trajectory of a momentum starts at x0 with exactly that momentum.
Per momentum: p, then the fractions [left | right][surface] without a correction, with EDC, and of the DVR run.  Printed for information:
surface hopping, corrected or not, is a method with an error of its own, and nothing here bounds it.  Run on a GPU box:
    python examples/hopping_decoherence.py [n_per_group] [n_momenta]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import gaussian_process_liouville_equation_amd as pkg  # noqa: E402
from gaussian_process_liouville_equation_amd import exact, hopping  # noqa: E402

n_per_group = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
n_E = int(sys.argv[2]) if len(sys.argv) > 2 else 16
UPPER, P0 = 1, 10.0
ln_e = float(np.log(P0 ** 2 / 2.0 / 2000.0))
s = exact.setup(ln_e, boundary=exact.ABSORBING)
momenta = np.linspace(s["p0"] - 3.0 * s["sigma_p"], s["p0"] + 3.0 * s["sigma_p"], n_E) if n_E > 1 else np.array([s["p0"]])
api = pkg.open_api(0)
lowest_packet = exact.initial_adiabatic_psi
try:
    runs = {}
    for label, decoherence in (("FSSH", None), ("EDC", "edc")):
        res = runs[label] = hopping.scan(api, model=hopping.ECR, num_pes=2, momenta=momenta, n_per_group=n_per_group, seed=1, fixed=True, surface0=UPPER,
                                         decoherence=decoherence)
        print(f"{label}: {n_E} momenta x {n_per_group} trajectories, dt = {res['dt'].min():g} ... {res['dt'].max():g}, {res['steps']} steps, "
              f"{res['hops'].mean():.3g} hops per trajectory; {res['total_seconds']:.2f} s")
    # the same packet on the upper surface for the DVR run, and the energies of the momenta above that surface at x0
    exact.initial_adiabatic_psi = lambda x, *rest: np.roll(lowest_packet(x, *rest), UPPER * len(x))
    e_upper = float(np.asarray(api.pes_adiabatic_n(2, exact.ECR, np.array([s["x"][int(np.argmin(np.abs(s["x"] - s["x0"])))]]))[0]).reshape(-1)[UPPER])
    dvr = exact.run(api, model=exact.ECR, num_pes=2, boundary=exact.ABSORBING, ln_energy=ln_e, write_phase=None, flux=True, until_absorbed=True,
                    spectrum=momenta ** 2 / 2.0 / s["mass"] + e_upper)
    print(f"DVR:  spectrum of {n_E} energies over 2^{dvr['spectrum_levels']} steps, {dvr['total_seconds'] + dvr['spectrum_seconds']:.2f} s")
    rho = dvr["spectrum"][:, 1:]
    held = rho.sum(axis=1) > 1e-3 * rho.sum(axis=1).max()  # energies the packet hardly holds have no DVR figure
    print("p | FSSH left 0, left 1, right 0, right 1 | with EDC (+- largest standard error) | DVR the same channels")
    for g in range(n_E):
        plain, edc = (" ".join(exact.fmt(v) for v in runs[label]["scattered"][g].reshape(-1)) for label in ("FSSH", "EDC"))
        exact_part = " ".join(exact.fmt(v) for v in rho[g] / rho[g].sum()) if held[g] else "-"
        print(f"{exact.fmt(momenta[g])} | {plain} | {edc} (+- {exact.fmt(runs['EDC']['stderr'][g].max())}) | {exact_part}")
finally:
    exact.initial_adiabatic_psi = lowest_packet
    api.close()
