"""Your own surfaces: two potentials that are not in the library, tabulated with pes.tabulate and registered with Api.pes_define, then a short
exact DVR run and a short exact MQCLE run on each.  Two levels: a dual avoided crossing with constants of its own and a
tilted lower surface; three levels: a variation on the library's TSAC with all three couplings and a bump on the middle level.  Run on a GPU box:
    python examples/custom_pes.py [table spacing, default 1/16]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import gaussian_process_liouville_equation_amd as pkg  # noqa: E402
from gaussian_process_liouville_equation_amd import exact, exact_mqcl, pes  # noqa: E402


def dual_crossing(x):
    """(V, dV/dx) at one position: V00 = T tanh(x / 2), V11 = E - A exp(-B x^2), V01 = C exp(-D x^2)"""
    A, B, C, D, E, T = 0.08, 0.35, 0.012, 0.09, 0.04, 0.002
    V = np.array([[T * np.tanh(0.5 * x), C * np.exp(-D * x * x)], [C * np.exp(-D * x * x), E - A * np.exp(-B * x * x)]])
    dV = np.array([[0.5 * T / np.cosh(0.5 * x) ** 2, -2 * C * D * x * np.exp(-D * x * x)],
                   [-2 * C * D * x * np.exp(-D * x * x), 2 * A * B * x * np.exp(-B * x * x)]])
    return V, dV


def three_crossings(x):
    """(V, dV/dx) at one position: +-A tanh(B x) outside, a Gaussian bump in the middle, sech couplings between all three"""
    A, B, C, D = 0.03, 0.6, 0.006, 0.4
    t, g, th = np.tanh(B * x), 1.0 / np.cosh(D * x), np.tanh(D * x)
    V, dV = np.zeros((3, 3)), np.zeros((3, 3))
    V[0, 0], V[1, 1], V[2, 2] = A * t, 0.004 * np.exp(-0.2 * x * x), -A * t
    dV[0, 0], dV[1, 1], dV[2, 2] = A * B * (1 - t * t), -0.0016 * x * np.exp(-0.2 * x * x), -A * B * (1 - t * t)
    for i, j, c in ((0, 1, C), (1, 2, 1.5 * C), (0, 2, 0.3 * C)):
        V[i, j] = V[j, i] = c * g
        dV[i, j] = dV[j, i] = -c * D * g * th
    return V, dV


spacing = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0 / 16
LN_E = -2.0  # total energy e^-2 Hartree, p0 = 23.3; grids and steps are the solvers' own defaults, and both runs end when the packet has passed
api = pkg.open_api(0)
try:
    for num_pes, surfaces in ((2, dual_crossing), (3, three_crossings)):
        # the table covers [-16, 16]; beyond it the library continues every entry along its tangent (these surfaces are flat there)
        model = api.pes_define(num_pes, *pes.tabulate(surfaces, -16.0, spacing, int(round(32.0 / spacing)) + 1))
        x = np.linspace(-4.0, 4.0, 5)
        E = api.pes_adiabatic_n(num_pes, model, x)[0]
        print(f"{surfaces.__name__}: model id {model}, {num_pes} levels; adiabatic energies at x = -4 ... 4:")
        print(np.array2string(E.T, precision=6, suppress_small=True))
        dvr = exact.run(api, model=model, num_pes=num_pes, boundary=exact.PERIODIC, ln_energy=LN_E, max_outputs=80)
        print(f"  DVR   ({dvr['setup']['n_grids']} grid points, {len(dvr['records'])} outputs, t = {dvr['records'][-1]['t']:g}): populations",
              np.array2string(dvr["records"][-1]["populations"], precision=6), "|", dvr["final_line"])
        mq = exact_mqcl.run(api, model=model, num_pes=num_pes, ln_energy=LN_E, write_phase=None, max_outputs=80)
        print(f"  MQCLE ({mq['setup']['n_grids']} x {mq['setup']['n_grids']} grid, {len(mq['records'])} outputs, t = {mq['records'][-1]['t']:g}): populations",
              np.array2string(mq["records"][-1]["populations"], precision=6), "|", mq["final_line"])
        api.pes_undefine(model)
finally:
    api.close()
