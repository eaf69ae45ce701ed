"""The cases in which the two exact solvers of the library meet (tests/test_scatter_dvr_host.py, tests/test_gpu_scatter_dvr.py; DESIGN.md §18,
"The two exact solvers against each other") and the figures recorded from the host run — a helper, not collected by pytest.

One side is the coupled-channel march (gple_scatter; tests/scatter_numpy.py): time independent, the asymptotes matched exactly.  The other is
the absorbing DVR chain (gple_dvr_hamiltonian, gple_dvr_absorber, gple_dvr_spectrum, gple_dvr_flux; tests/dvr_spectrum_numpy.py,
tests/dvr_flux_numpy.py): one clocked packet, what each channel (side of the box x adiabatic surface) absorbed per total energy.  They share no
code, and nothing but the physics makes them agree on which index is the incoming surface, how [left | right][surface] is ordered, where the
zero of the total energy lies and how flux is normalised.

A case: the model (a built-in id; table=True: tabulated at dx = 1 / 16 on [-40, 40] and given to both solvers as one user table), the levels,
the physical box [-box, box] of the DVR grid, dx, dt (after the halving rule of dvr_absorbing_numpy.halve, asserted), the absorber's length as
a multiple of the driver's 2 pi hbar / (p0 - 3 sigma_p), J (2^J steps are transformed), the packet (x0, p0, sigma_p, the incoming adiabatic
surface), nine momenta in p0 +- 1.5 sigma_p with E = p^2 / 2m + eps_surface(-exact_box), the rule of scattering.run, and exact_box, the box of
the march the DVR figures are held to: the DVR box where the potential is flat beyond it (asserted against the march on +-40), else +-40 itself,
because the DVR grid sees the potential untruncated.  n_left comes with the grid: the points left of the box's centre.

RECORDED holds per case what the host run measured, all on the CPU with the restatements alone (float64 march against complex128 spectrum):
    all         the largest gap over the 2 num_pes channels between a_c / sum_c a_c and the march's column
    transmitted the largest gap of the transmitted branching ratios T_j / sum_j T_j
    reflection  the spurious reflection: the largest reflected fraction of the DVR side beyond the march's own
    packet      the largest gap per channel of the flux line (dvr_flux_numpy forms on psi0, times dx) from scattering.packet_line
    D           the largest distance between the float64 and the long double march (the rounding floor of the exact side)
    S           a bound of sum_{k < K} |psi_k| from the norms at the powers of two (|psi_k| does not grow)
The host test asserts that each of the first four is reproduced from both sides (measured <= 1.25 recorded and >= recorded / 4), so a record
can be neither stale nor padded; D and S are bounds and are held from above and from a quarter below as well."""
import functools
import math

import numpy as np

from gaussian_process_liouville_equation_amd import pes
from tests import dvr_numpy as DN
from tests import hop_numpy as HN

HBAR = 1.0
MASS, DX, DT_MAX, SIGMA_P = 2000.0, 1.0 / 16.0, 1.0 / 8.0, 1.0
WIDE = 40.0                 # the box on which every potential here is flat to rounding
KH = 0.1                    # the march's grid: the smallest n_steps with k_max h <= 0.1
DENSITY_THRESHOLD = 0.1     # every energy of a case carries at least this much of the peak of sum_c a_c
REMAINING_MAX = 2e-3        # |P^K psi0|^2 dx
TEETH = 100.0               # a corrupted comparison must miss by this many bounds
TABLE_BOX, TABLE_DX = 40.0, 1.0 / 16.0

CASES = {
    "sac-lower": dict(model=HN.SAC, num_pes=2, box=8.0, dt=1.0 / 8.0, absorber=4, J=16, x0=-5.0, p0=20.0, surface=0, exact_box=8.0),
    "sac-upper": dict(model=HN.SAC, num_pes=2, box=8.0, dt=1.0 / 8.0, absorber=4, J=16, x0=-5.0, p0=20.0, surface=1, exact_box=8.0),
    "sac-driver-absorber": dict(model=HN.SAC, num_pes=2, box=8.0, dt=1.0 / 8.0, absorber=1, J=16, x0=-5.0, p0=20.0, surface=0, exact_box=8.0),
    "dac": dict(model=HN.DAC, num_pes=2, box=12.0, dt=1.0 / 16.0, absorber=4, J=17, x0=-8.0, p0=25.0, surface=0, exact_box=WIDE),
    "tsac": dict(model=HN.TSAC, num_pes=3, box=12.0, dx=3.0 / 32.0, dt=1.0 / 8.0, absorber=4, J=16, x0=-8.0, p0=20.0, surface=0, exact_box=WIDE),
    "dac-table": dict(model=HN.DAC, num_pes=2, box=12.0, dt=1.0 / 16.0, absorber=4, J=17, x0=-8.0, p0=25.0, surface=0, exact_box=WIDE, table=True),
}
for _c in CASES.values():
    _c.setdefault("table", False)
    _c.setdefault("dx", DX)
    _c.update(mass=MASS, sigma_p=SIGMA_P)

# measured by tests/test_scatter_dvr_host.py on the CPU (see the module's text), rounded upwards to three digits
RECORDED = {
    "sac-lower": dict(all=1.34e-06, transmitted=1.3e-06, reflection=9.13e-08, packet=1.41e-05, D=4.54e-14, S=65680.9),
    "sac-upper": dict(all=1.16e-06, transmitted=1.15e-06, reflection=1.45e-07, packet=1.15e-05, D=4.17e-14, S=65557.5),
    "sac-driver-absorber": dict(all=0.00386, transmitted=0.00275, reflection=0.00265, packet=0.00111, D=4.54e-14, S=68243.1),
    "dac": dict(all=0.000556, transmitted=0.000556, reflection=4.75e-07, packet=0.000216, D=1.7e-12, S=135447.0),
    "tsac": dict(all=0.00315, transmitted=0.00315, reflection=6.04e-06, packet=0.000779, D=4.41e-13, S=104979.0),
    "dac-table": dict(all=0.000556, transmitted=0.000556, reflection=4.75e-07, packet=0.000216, D=1.85e-12, S=135447.0),
}

# reciprocity, T_{j<-i}(V) = T_{i<-j}(V mirrored): the models on their boxes with N = 1500 and 70 momenta in [3, 30] above the higher of the two
# ends' lowest thresholds; `least`: the entries that must have been compared (both sides finite), so NaN columns cannot hollow the test out
RECIPROCITY_STEPS, RECIPROCITY_MOMENTA = 1500, (3.0, 30.0, 70)
RECIPROCITY = {
    "ecr": dict(model=HN.ECR, num_pes=2, box=40.0, least=150),
    "sac": dict(model=HN.SAC, num_pes=2, box=40.0, least=232),
    "tsac": dict(model=HN.TSAC, num_pes=3, box=30.0, least=457),
}
# per case on the CPU: g (the largest gap, float64 march) and D, D_mirror (float64 against long double) for the built-in functions and for
# their tables at dx = 1 / 16, which is what the device runs
RECIPROCITY_RECORDED = {
    "ecr": dict(function=dict(g=4.47e-13, D=4.54e-13, D_mirror=4.36e-14), table=dict(g=7.23e-13, D=7.21e-13, D_mirror=4.58e-14)),
    "sac": dict(function=dict(g=2.3e-14, D=4.45e-14, D_mirror=4.61e-14), table=dict(g=2.64e-14, D=6.66e-14, D_mirror=5.58e-14)),
    "tsac": dict(function=dict(g=2.86e-14, D=2.55e-13, D_mirror=2.45e-13), table=dict(g=3.55e-14, D=1.61e-13, D_mirror=1.76e-13)),
}


# ---- geometry: what both sides derive from a case without solving anything -----------------------------------------------------------------------
def momenta(c):
    return np.linspace(c["p0"] - 1.5 * c["sigma_p"], c["p0"] + 1.5 * c["sigma_p"], 9)


def peak_momenta(c):
    """49 momenta over p0 +- 3 sigma_p, the case's nine among them: where the peak of the density is looked for"""
    return np.linspace(c["p0"] - 3.0 * c["sigma_p"], c["p0"] + 3.0 * c["sigma_p"], 49)


def energies_of(c, eps_in, p=None):
    """E = p^2 / 2m + eps_in, eps_in the adiabatic energy of the incoming surface at -exact_box: the rule of scattering.run"""
    p = momenta(c) if p is None else p
    return p * p / 2.0 / c["mass"] + eps_in


def geometry(c):
    """the grid of exact.setup(boundary=ABSORBING) with the absorber's length scaled: length, n_abs, n, x, n_left, sigma_x"""
    length = c["absorber"] * 2.0 * math.pi * HBAR / (c["p0"] - 3.0 * c["sigma_p"])
    n_abs = int(length / c["dx"])
    n = int(2.0 * c["box"] / c["dx"]) + 1 + 2 * n_abs
    x = -c["box"] + c["dx"] * (np.arange(n) - n_abs)
    return dict(length=length, n_abs=n_abs, n=n, dim=c["num_pes"] * n, x=x, n_left=int(np.sum(x < 0.0)), sigma_x=HBAR / 2.0 / c["sigma_p"])


def packet(c, g, basis):
    """psi0 = basis[:, j, surface] times the normalised Gaussian, diabatic, from the adiabatic states `basis` (n, N, N) of the grid"""
    wave = DN.gaussian(g["x"], c["x0"], c["p0"], g["sigma_x"])
    return np.concatenate([basis[:, j, c["surface"]] * wave for j in range(c["num_pes"])])


def march_steps(c, e_max, lowest, box):
    """the smallest n_steps with k_max h <= KH on [-box, box] (scattering.default_steps)"""
    k_max = math.sqrt(max(2.0 * c["mass"] * (e_max - lowest), 0.0)) / HBAR
    return max(2, int(math.ceil(k_max * 2.0 * box / KH)))


@functools.lru_cache(maxsize=None)
def model_table(model, num_pes, box=TABLE_BOX):
    """pes.tabulate of a built-in model on [-box, box] at dx = 1 / 16: the DVR grids here are subsets of its nodes"""
    n = int(round(2.0 * box / TABLE_DX)) + 1
    return HN.FunctionTable(*pes.tabulate(HN.scalar_function(HN.builtin(model, num_pes)), -box, TABLE_DX, n))


def mirrored(tab):
    """the table of V(-x) on the same symmetric nodes: V and dV reversed, dV negated"""
    assert tab.x_first == -(tab.x_first + tab.dx * (tab.V.shape[0] - 1))
    return HN.FunctionTable(tab.x_first, tab.dx, tab.V[::-1].copy(), -tab.dV[::-1])


# ---- the figures of a comparison, from the two sides' outputs: shared by the host and the device test ------------------------------------------------
def fractions(a):
    """a (n_E, 2 N) -> a_c / sum_c a_c"""
    return a / a.sum(axis=1, keepdims=True)


def branching(columns, num_pes):
    """(n_E, 2 N) [left | right][surface] -> the transmitted branching ratios T_j / sum_j T_j (n_E, N)"""
    T = columns[:, num_pes:]
    return T / T.sum(axis=1, keepdims=True)


def gaps(a, exact, num_pes):
    """(all, transmitted, reflection) of DVR densities a (n_E, 2 N) against the march's columns exact (n_E, 2 N)"""
    f = fractions(a)
    return (float(np.abs(f - exact).max()), float(np.abs(branching(a, num_pes) - branching(exact, num_pes)).max()),
            float((f[:, :num_pes] - exact[:, :num_pes]).max()))


def reproduces(measured, recorded):
    """neither stale nor padded"""
    return recorded / 4.0 <= measured <= 1.25 * recorded


def reciprocity_energies(lowest_left, lowest_right):
    """the energies of 70 momenta in [3, 30] on the lowest surface of the left end that lie above the higher of the two ends' lowest thresholds"""
    p = np.linspace(*RECIPROCITY_MOMENTA)
    E = p * p / 2.0 / MASS + lowest_left
    return E[E > max(lowest_left, lowest_right)]


def reciprocity_gap(forward, backward):
    """(the largest |T_{j<-i}(V) - T_{i<-j}(mirror)| where both are finite, the number of entries compared) of two prob arrays"""
    a, b = forward[:, :, 1, :], np.swapaxes(backward[:, :, 1, :], 1, 2)
    both = np.isfinite(a) & np.isfinite(b)
    return float(np.abs(a[both] - b[both]).max()), int(both.sum())
