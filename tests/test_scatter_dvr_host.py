"""CPU, restatements only: the coupled-channel march (tests/scatter_numpy.py) against the spectrum and the flux line of the absorbing DVR chain
(tests/dvr_spectrum_numpy.py, tests/dvr_flux_numpy.py) on the cases of tests/scatter_dvr_cases.py, and transmission reciprocity of the march.
The two solvers share no code and no convention ("The two exact solvers against each other").  Every figure is printed, and held
to its record in the cases file from both sides: measured <= 1.25 recorded and >= recorded / 4.  The conditions under which the comparison means
anything are asserted, not tuned around: every energy carries a tenth of the peak density, at most 2e-3 of the packet is left in the box, the box
of the march is flat (against +-40), and the long double march agrees with the float64 one to 1e-10."""
import functools

import numpy as np
import pytest

from gaussian_process_liouville_equation_amd import scattering
from tests import dvr_absorbing_numpy as AN
from tests import dvr_flux_numpy as FN
from tests import dvr_numpy as DN
from tests import dvr_spectrum_numpy as SP
from tests import hop_numpy as HN
from tests import scatter_dvr_cases as SD
from tests import scatter_numpy as SN


def potential(c):
    return HN.table(SD.model_table(c["model"], c["num_pes"])) if c["table"] else HN.builtin(c["model"], c["num_pes"])


@functools.lru_cache(maxsize=None)
def operators(model, num_pes, box, dx, absorber, p0, J):
    """what the DVR side of a case does not owe to its packet, once for the cases that share it (the two SAC surfaces; DAC and its table, whose
    nodes on this grid are the function's own values): H of tests/dvr_numpy.py, W, dt after the halving rule, the adiabatic basis, the
    one-step propagator P and the flux forms G_c of 2^J steps"""
    c = dict(num_pes=num_pes, box=box, dx=dx, absorber=absorber, p0=p0, sigma_p=SD.SIGMA_P)
    g = SD.geometry(c)
    x = g["x"]
    V = HN.builtin(model, num_pes)(x)[0]
    H = DN.hamiltonian(num_pes, model, DN.REFLECTIVE, x[0], dx, g["n"], SD.MASS)
    a = np.arange(g["n"])
    blocks = np.stack([[H[i * g["n"] + a, j * g["n"] + a] for j in range(num_pes)] for i in range(num_pes)]).transpose(2, 0, 1)
    kinetic = (np.pi / dx) ** 2 / 6.0 / SD.MASS
    assert np.abs(blocks - kinetic * np.eye(num_pes) - V).max() <= 4.0 * np.finfo(float).eps * kinetic  # H holds this potential
    basis = np.ascontiguousarray(HN.sign_convention(HN.jacobi(V)[1]))
    W = AN.absorber(x, SD.MASS, -box, box, g["length"])
    dt, _ = AN.halve(SD.DT_MAX, W)
    P = AN.p4(AN.generator(H, W, num_pes, dt))
    _, G = FN.recurrence(P, FN.channels(FN.loss(P), basis, g["n_left"]), 2 ** J)
    return dict(V=V, H=H, W=W, dt=dt, basis=basis, P=P, G=G)


def norm_sum_bound(P, psi0, J):
    """S >= sum_{k < 2^J} |P^k psi0|: the steps 2^j ... 2^(j + 1) - 1 weigh at most what step 2^j has, because |psi_k| does not grow"""
    R, total, last = P, float(np.linalg.norm(psi0)), float(np.linalg.norm(psi0))
    for j in range(J):
        if j:
            R = AN.cmul(R, R)
        now = float(np.linalg.norm(R @ psi0))
        assert now <= last * (1.0 + 1e-12)
        total, last = total + 2.0 ** j * now, now
    return total


@functools.lru_cache(maxsize=None)
def solve(name):
    """one case through both restatements, once"""
    c = SD.CASES[name]
    g, N, pot = SD.geometry(c), c["num_pes"], potential(c)
    x, eb = g["x"], c["exact_box"]
    op = operators(c["model"], N, c["box"], c["dx"], c["absorber"], c["p0"], c["J"])
    if c["table"]:  # the grid's points are nodes of the table, and the nodes are the function's values
        assert np.array_equal(pot(x)[0], op["V"])
    H, W, dt, basis = op["H"], op["W"], op["dt"], op["basis"]
    psi0 = SD.packet(c, g, basis)
    ends = np.array([HN.jacobi(pot(np.array([e]))[0])[0][0] for e in (-eb, eb)])
    E = SD.energies_of(c, ends[0, c["surface"]])
    # beside the case's energies, 49 over the packet's whole range: the peak of the density, for the threshold
    fine = SD.energies_of(c, ends[0, c["surface"]], SD.peak_momenta(c))
    _, a, left = SP.restated(H, W, N, dt, psi0, np.concatenate([E, fine]), c["J"], basis, g["n_left"])
    a, peak = a[:len(E)], float(a.sum(axis=1).max())
    S = norm_sum_bound(op["P"], psi0, c["J"])
    line = FN.forms(op["G"], psi0) * c["dx"]
    steps = SD.march_steps(c, float(E.max()), float(ends.min()), eb)
    ref = SN.march(pot, N, c["mass"], -eb, eb, steps, E)
    wide = SN.march(pot, N, c["mass"], -eb, eb, steps, E, dtype=np.longdouble)
    D = float(np.nanmax(np.abs((ref["prob"] - wide["prob"]).astype(np.float64))))
    far = None
    if eb != SD.WIDE:
        far = SN.march(pot, N, c["mass"], -SD.WIDE, SD.WIDE, SD.march_steps(c, float(E.max()), float(ends.min()), SD.WIDE), E)["prob"][:, c["surface"]].reshape(len(E), -1)
    api = SN.NumpyScatterApi({c["model"]: pot})
    average = scattering.packet_line(api, model=c["model"], num_pes=N, p0=c["p0"], sigma_p=c["sigma_p"], surface0=c["surface"], x_left=-eb, x_right=eb,
                                     mass=c["mass"]).reshape(-1)
    return dict(case=c, geometry=g, dt=dt, energies=E, a=a, peak=peak, remaining=left * c["dx"], S=S, line=line, steps=steps,
                exact=ref["prob"][:, c["surface"]].reshape(len(E), -1), defect=ref["defect"][:, c["surface"]], D=D, far=far, average=average, ends=ends)


# ---- 1. the two solvers, per case ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SD.CASES))
def test_spectrum_against_the_march(name):
    s, rec = solve(name), SD.RECORDED[name]
    c, N = s["case"], s["case"]["num_pes"]
    every, transmitted, reflection = SD.gaps(s["a"], s["exact"], N)
    weakest = float(s["a"].sum(axis=1).min() / s["peak"])
    print(f"{name}: dim {s['geometry']['dim']}, dt {s['dt']}, J {c['J']}, march N = {s['steps']} on +-{c['exact_box']:g}; all channels {every:.3g} "
          f"(recorded {rec['all']:.3g}), transmitted ratios {transmitted:.3g} ({rec['transmitted']:.3g}), spurious reflection {reflection:.3g} "
          f"({rec['reflection']:.3g}); weakest energy {weakest:.3g} of the peak, remaining {s['remaining']:.3g}, D {s['D']:.3g} ({rec['D']:.3g}), "
          f"S {s['S']:.6g} ({rec['S']:.6g}), largest |defect| {np.abs(s['defect']).max():.3g}")
    assert s["dt"] == c["dt"]                                                # the halving rule
    assert np.isfinite(s["exact"]).all() and (s["exact"] > 0.0).all()        # every channel open at every energy
    assert weakest >= SD.DENSITY_THRESHOLD                                   # none left out
    assert s["remaining"] <= SD.REMAINING_MAX
    assert s["D"] <= 1e-10 and np.abs(s["defect"]).max() < 1e-11
    if s["far"] is not None:                                                 # the march's box is flat
        flat = float(np.abs(s["far"] - s["exact"]).max())
        print(f"{name}: the march on +-{c['exact_box']:g} against +-{SD.WIDE:g}: {flat:.3g}, a tenth of the recorded gap {rec['all'] / 10.0:.3g}")
        assert flat <= rec["all"] / 10.0
    for key, value in (("all", every), ("transmitted", transmitted), ("reflection", reflection), ("D", s["D"]), ("S", s["S"])):
        assert SD.reproduces(value, rec[key]), (name, key, value, rec[key])


@pytest.mark.parametrize("name", list(SD.CASES))
def test_flux_line_against_the_packet_average(name):
    """what the absorber took of the whole packet, per channel, against the Gaussian-momentum average of the march's columns: the gap is bounded
    by the spurious reflection, what is left in the box and the transmitted gap, and is recorded like the others"""
    s, rec = solve(name), SD.RECORDED[name]
    gap = float(np.abs(s["line"] - s["average"]).max())
    print(f"{name}: flux line {' '.join('%.6g' % v for v in s['line'])}, packet average {' '.join('%.6g' % v for v in s['average'])}, gap {gap:.3g} "
          f"(recorded {rec['packet']:.3g}), absorbed {s['line'].sum():.6f} + remaining {s['remaining']:.3g}")
    assert abs(s["line"].sum() + s["remaining"] - 1.0) <= 1e-9
    assert SD.reproduces(gap, rec["packet"]), (name, gap, rec["packet"])


def test_the_comparison_has_teeth():
    """two misreadings the comparison has to see, on sac-lower: the energies without eps_surface0, and the two transmitted columns swapped"""
    s, rec = solve("sac-lower"), SD.RECORDED["sac-lower"]
    c, pot = s["case"], potential(s["case"])
    eb = c["exact_box"]
    no_zero = SN.march(pot, 2, c["mass"], -eb, eb, s["steps"], SD.energies_of(c, 0.0))["prob"][:, 0].reshape(9, -1)
    shifted = SD.gaps(s["a"], no_zero, 2)[1]
    swapped = SD.gaps(s["a"], s["exact"][:, [0, 1, 3, 2]], 2)[1]
    print(f"sac-lower: recorded transmitted gap {rec['transmitted']:.3g}; without eps_surface0 {shifted:.3g} ({shifted / rec['transmitted']:.3g} x), "
          f"columns swapped {swapped:.3g} ({swapped / rec['transmitted']:.3g} x)")
    assert s["ends"][0, 0] < -0.009                                          # the zero that is dropped is not zero
    assert shifted > SD.TEETH * rec["transmitted"] and swapped > SD.TEETH * rec["transmitted"]


# ---- 2. reciprocity of the march ----------------------------------------------------------------------------------------------------------------------
def reciprocity(pot, mirror, num_pes, box, dtype=np.float64):
    lowest = [HN.jacobi(pot(np.array([e]))[0])[0][0][0] for e in (-box, box)]
    E = SD.reciprocity_energies(*lowest)
    args = (num_pes, SD.MASS, -box, box, SD.RECIPROCITY_STEPS, E)
    one, other = SN.march(pot, *args, dtype=dtype), SN.march(mirror, *args, dtype=dtype)
    return E, one["prob"], other["prob"]


@pytest.mark.parametrize("tabulated", [False, True], ids=["function", "table"])
@pytest.mark.parametrize("name", list(SD.RECIPROCITY))
def test_transmission_reciprocity(name, tabulated):
    r = SD.RECIPROCITY[name]
    rec = SD.RECIPROCITY_RECORDED[name]["table" if tabulated else "function"]
    if tabulated:
        tab = SD.model_table(r["model"], r["num_pes"], r["box"])
        pot, mirror = HN.table(tab), HN.table(SD.mirrored(tab))
    else:
        pot = HN.builtin(r["model"], r["num_pes"])
        mirror = lambda x: pot(-x)[0]
    E, one, other = reciprocity(pot, mirror, r["num_pes"], r["box"])
    _, wide_one, wide_other = reciprocity(pot, mirror, r["num_pes"], r["box"], dtype=np.longdouble)
    g, count = SD.reciprocity_gap(one, other)
    D = float(np.nanmax(np.abs((one - wide_one).astype(np.float64))))
    D_mirror = float(np.nanmax(np.abs((other - wide_other).astype(np.float64))))
    print(f"reciprocity {name} {'table' if tabulated else 'function'}: {len(E)} energies, {count} entries compared, g {g:.3g} (recorded {rec['g']:.3g}), "
          f"D {D:.3g} ({rec['D']:.3g}), D of the mirror {D_mirror:.3g} ({rec['D_mirror']:.3g}), long double g {SD.reciprocity_gap(wide_one, wide_other)[0]:.3g}")
    assert count >= r["least"]
    for key, value in (("g", g), ("D", D), ("D_mirror", D_mirror)):
        assert SD.reproduces(value, rec[key]), (name, key, value, rec[key])
