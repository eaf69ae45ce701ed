"""GPU: the two exact solvers of the library against each other ("The two exact solvers against each other").  The coupled-channel
march (gple_scatter, scattering.packet_line) and the absorbing DVR chain (gple_dvr_hamiltonian, gple_dvr_absorber, gple_dvr_spectrum,
gple_dvr_flux + gple_dvr_flux_apply) share no code, no clock and no asymptote, and nothing but the physics makes them agree on the incoming
surface's index, the order [left | right][surface], the zero of the total energy and the flux weights.  No restatement runs here: the cases and
the host's recorded figures come from tests/scatter_dvr_cases.py (asserted on the CPU by tests/test_scatter_dvr_host.py), and device is held to
device within

    the recorded host figure  +  the spectrum's parity tolerance  +  the march's parity tolerance,        no further factor

the two tolerances carried to the quantity compared:
    density entries   t_a = 8 (J + 1) eps sqrt(dim) S^2 (tests/test_gpu_dvr_spectrum.py's driver test), S recorded from the host run; a fraction
                      a_c / sum_c a_c moves by at most t_a (1 + 2 N) / sum_c a_c, a transmitted ratio by t_a (1 + N) / sum_j a_(right, j)
    prob entries      t_s = 64 D + 1e-13 (tests/test_gpu_scatter.py), D recorded from the host run; a column as it is, a transmitted ratio
                      by t_s (1 + N) / sum_j T_j, the packet average (weights that sum to one) by t_s
    flux line         8 (J + 1) eps sqrt(dim) S |psi0| dx: a form sums psi_k^H D_c psi_k over the steps, sum_k |psi_k|^2 <= S |psi0|
Every figure is printed before it is asserted; the ratios measured on the MI355X are in DESIGN.md §18.

Reciprocity, T_{j<-i}(V) = T_{i<-j}(V mirrored), ties the incoming index, the final index and the flux weights s^L / s^R of gple_scatter together
on device output alone: a table and its mirror (V and dV reversed, dV negated) are one discrete problem read from the other end."""
import math

import numpy as np
import pytest

from gaussian_process_liouville_equation_amd import scattering
from tests import scatter_dvr_cases as SD

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
REFLECTIVE = 0
_solved = {}


class defined:
    """a user potential on the session's context for the length of a with block"""

    def __init__(self, gpu, tab):
        self.gpu, self.tab = gpu, tab

    def __enter__(self):
        t = self.tab
        self.model = self.gpu.pes_define(t.num_pes, t.x_first, t.dx, t.V, t.dV)
        return self.model

    def __exit__(self, *exc):
        self.gpu.pes_undefine(self.model)


def both_solvers(gpu, c, model):
    g, N = SD.geometry(c), c["num_pes"]
    x, n, eb = g["x"], g["n"], c["exact_box"]
    H, _, basis = gpu.dvr_hamiltonian(N, model, REFLECTIVE, x[0], c["dx"], n, c["mass"])
    W = gpu.dvr_absorber(x[0], c["dx"], n, c["mass"], -c["box"], c["box"], g["length"])
    dt = SD.DT_MAX
    while dt * float(W.max()) / SD.HBAR > 2.0:  # the halving rule of exact.setup
        dt /= 2.0
    psi0 = SD.packet(c, g, basis)
    ends = scattering.end_energies(gpu, N, model, -eb, eb)
    eps_in = float(ends[0, c["surface"]])
    E = SD.energies_of(c, eps_in)
    fine = SD.energies_of(c, eps_in, SD.peak_momenta(c))
    density, _, left = gpu.dvr_spectrum(N, n, H, W, dt, c["J"], basis, g["n_left"], psi0, np.concatenate([E, fine]))
    density = density.reshape(len(density), -1)
    _, G = gpu.dvr_flux(N, n, H, W, dt, 2 ** c["J"], basis, g["n_left"], device_out=True, want_u=False)
    line = gpu.dvr_flux_apply(N, n, G, psi0)[0].reshape(-1) * c["dx"]
    del G
    steps = SD.march_steps(c, float(E.max()), float(ends.min()), eb)
    prob, defect = gpu.scatter(N, model, c["mass"], -eb, eb, steps, E)
    average = scattering.packet_line(gpu, model=model, num_pes=N, p0=c["p0"], sigma_p=c["sigma_p"], surface0=c["surface"], x_left=-eb, x_right=eb,
                                     mass=c["mass"]).reshape(-1)
    return dict(case=c, geometry=g, dt=dt, eps_in=eps_in, a=density[:len(E)], peak=float(density.sum(axis=1).max()), remaining=left * c["dx"], line=line,
                norm0=float(np.linalg.norm(psi0)), steps=steps, prob=prob, exact=prob[:, c["surface"]].reshape(len(E), -1), defect=defect[:, c["surface"]],
                average=average)


def solve(gpu, name):
    """one case through both solvers on the device, once per module"""
    if name not in _solved:
        c = SD.CASES[name]
        if c["table"]:
            with defined(gpu, SD.model_table(c["model"], c["num_pes"])) as model:
                _solved[name] = both_solvers(gpu, c, model)
        else:
            _solved[name] = both_solvers(gpu, c, c["model"])
    return _solved[name]


def bounds(s, rec, exact=None):
    """(all channels, transmitted ratios, packet average): the recorded host figure plus the two parity tolerances, per energy where they depend
    on it; `exact`: the march's columns, where they are not the case's own"""
    c, N = s["case"], s["case"]["num_pes"]
    exact = s["exact"] if exact is None else exact
    t_a = 8.0 * (c["J"] + 1) * EPS * math.sqrt(s["geometry"]["dim"]) * rec["S"] ** 2
    t_s = 64.0 * rec["D"] + 1e-13
    every = rec["all"] + t_a * (1 + 2 * N) / s["a"].sum(axis=1) + t_s
    transmitted = rec["transmitted"] + t_a * (1 + N) / s["a"][:, N:].sum(axis=1) + t_s * (1 + N) / exact[:, N:].sum(axis=1)
    packet = rec["packet"] + 8.0 * (c["J"] + 1) * EPS * math.sqrt(s["geometry"]["dim"]) * rec["S"] * s["norm0"] * c["dx"] + t_s
    return every, transmitted, packet


def transmitted_gap(a, exact, N):
    """per energy: the largest gap of the transmitted branching ratios"""
    return np.abs(SD.branching(a, N) - SD.branching(exact, N)).max(axis=1)


# ---- 1. device against device ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SD.CASES))
def test_spectrum_and_flux_against_the_march(gpu, name):
    s, rec = solve(gpu, name), SD.RECORDED[name]
    c, N = s["case"], s["case"]["num_pes"]
    every, transmitted, packet = bounds(s, rec)
    f = SD.fractions(s["a"])
    gap_all = np.abs(f - s["exact"]).max(axis=1)
    gap_tr = transmitted_gap(s["a"], s["exact"], N)
    gap_packet = float(np.abs(s["line"] - s["average"]).max())
    reflection = float((f[:, :N] - s["exact"][:, :N]).max())
    weakest = float(s["a"].sum(axis=1).min() / s["peak"])
    print(f"{name}: dim {s['geometry']['dim']}, dt {s['dt']}, J {c['J']}, march N = {s['steps']} on +-{c['exact_box']:g}")
    print(f"{name}: all channels {gap_all.max():.3g} (host {rec['all']:.3g}), gap / bound {(gap_all / every).max():.3g}, tolerances' share of the bound "
          f"{(1.0 - rec['all'] / every).max():.3g}")
    print(f"{name}: transmitted ratios {gap_tr.max():.3g} (host {rec['transmitted']:.3g}), gap / bound {(gap_tr / transmitted).max():.3g}, tolerances' share "
          f"{(1.0 - rec['transmitted'] / transmitted).max():.3g}")
    print(f"{name}: flux line {' '.join('%.6g' % v for v in s['line'])}, packet average {' '.join('%.6g' % v for v in s['average'])}, gap {gap_packet:.3g} "
          f"(host {rec['packet']:.3g}), gap / bound {gap_packet / packet:.3g}")
    print(f"{name}: spurious reflection {reflection:.3g} (host {rec['reflection']:.3g}), weakest energy {weakest:.3g} of the peak, remaining {s['remaining']:.3g}, "
          f"largest |defect| {np.abs(s['defect']).max():.3g}")
    assert s["dt"] == c["dt"]                                                 # the halving rule, on the device's W
    assert np.isfinite(s["exact"]).all() and (s["exact"] > 0.0).all()         # every channel open at every energy
    assert weakest >= SD.DENSITY_THRESHOLD                                    # the conditions of the host, on the device's own output; none left out
    assert 0.0 <= s["remaining"] <= SD.REMAINING_MAX
    assert np.abs(s["defect"]).max() < 1e-11                                  # unitarity of the march where the fractions sum to one by construction
    assert (gap_all <= every).all()
    assert (gap_tr <= transmitted).all()
    assert gap_packet <= packet


# ---- 2. teeth ------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_comparison_has_teeth_on_the_device(gpu):
    """on sac-lower: the energies without eps_surface0, and the two transmitted columns swapped, each more than 100 bounds away"""
    s, rec = solve(gpu, "sac-lower"), SD.RECORDED["sac-lower"]
    c = s["case"]
    eb = c["exact_box"]
    prob, _ = gpu.scatter(2, c["model"], c["mass"], -eb, eb, s["steps"], SD.energies_of(c, 0.0))
    no_zero = prob[:, 0].reshape(9, -1)
    swapped_columns = s["exact"][:, [0, 1, 3, 2]]
    shifted = (transmitted_gap(s["a"], no_zero, 2) / bounds(s, rec, no_zero)[1]).max()
    swapped = (transmitted_gap(s["a"], swapped_columns, 2) / bounds(s, rec, swapped_columns)[1]).max()
    print(f"sac-lower on the device: eps_surface0 = {s['eps_in']:.6g}; without it the transmitted ratios miss by {shifted:.3g} bounds, columns swapped by "
          f"{swapped:.3g} bounds")
    assert s["eps_in"] < -0.009
    assert shifted > SD.TEETH and swapped > SD.TEETH


# ---- 3. reciprocity ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SD.RECIPROCITY))
def test_transmission_reciprocity_on_the_device(gpu, name):
    r, rec = SD.RECIPROCITY[name], SD.RECIPROCITY_RECORDED[name]["table"]
    N, box = r["num_pes"], r["box"]
    tab = SD.model_table(r["model"], N, box)
    with defined(gpu, tab) as model, defined(gpu, SD.mirrored(tab)) as mirror:
        ends = scattering.end_energies(gpu, N, model, -box, box)
        E = SD.reciprocity_energies(float(ends[0, 0]), float(ends[1, 0]))
        one, defect = gpu.scatter(N, model, SD.MASS, -box, box, SD.RECIPROCITY_STEPS, E)
        other, defect_mirror = gpu.scatter(N, mirror, SD.MASS, -box, box, SD.RECIPROCITY_STEPS, E)
    gap, count = SD.reciprocity_gap(one, other)
    tol = (64.0 * rec["D"] + 1e-13) + (64.0 * rec["D_mirror"] + 1e-13) + rec["g"]
    print(f"reciprocity {name}: {len(E)} energies, {count} entries compared, largest gap {gap:.3g}, gap / tolerance {gap / tol:.3g} (host g {rec['g']:.3g}), "
          f"largest |defect| {max(np.nanmax(np.abs(defect)), np.nanmax(np.abs(defect_mirror))):.3g}")
    assert count >= r["least"]
    assert gap <= tol
