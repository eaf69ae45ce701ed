"""GPU: the MQCLE spectral propagator (gple_mqcl_evolve, gple_mqcl_observe) against answers that are not its numpy restatement, on the family
V = k x^2 / 2 I + A + B x on which the MQCLE has no method error (tests/exact_cases.py): a closed form down to the Strang
splitting (B = 0, diagonal A), and the DVR chain of the same library (gple_dvr_hamiltonian, numpy.linalg.eigh on the host, gple_dvr_propagate,
gple_wigner), which shares no code and no reading of the reference with the propagator.  Nothing here runs a restatement: the bounds are the
project's 2e-12 for the closed form and the restatements' own figures (asserted in tests/test_solvers_agree_host.py, recorded in
exact_cases.COUPLED) with the margins of §12 for the cross-solver comparison.  Every figure is printed before it is asserted."""
import functools

import numpy as np
import pytest

from tests import exact_cases as XC

pytestmark = pytest.mark.gpu


class defined:
    """a user potential on the session's context for the length of a with block"""

    def __init__(self, gpu, num_pes, table):
        self.gpu, self.num_pes, self.table = gpu, num_pes, table

    def __enter__(self):
        self.model = self.gpu.pes_define(self.num_pes, *self.table)
        return self.model

    def __exit__(self, *exc):
        self.gpu.pes_undefine(self.model)


# ---- 1. the closed form ---------------------------------------------------------------------------------------------------------------------
closed_case = functools.lru_cache(maxsize=None)(XC.closed_case)  # start and answer are built once per (num_pes, n, lengths) and only read


@pytest.mark.parametrize("table", ["grid", "coarse"])
@pytest.mark.parametrize("driver_lengths", [False, True], ids=["n-spacings", "driver-lengths"])
@pytest.mark.parametrize("n", sorted(XC.CLOSED_GRIDS))
@pytest.mark.parametrize("num_pes", [2, 3])
def test_closed_form(gpu, num_pes, n, driver_lengths, table):
    """every element a <= b rides the harmonic flow of the Strang map (both shears scaled by n / (n - 1) under the driver's lengths, quirk 1)
    and turns at its own gap; M = 128 at NT = 64 (n = 64), an odd n (127), the last n on NT = 64 (128) and NT = 256 (257, 300)"""
    x, p, (length_x, length_p), _, start, expected = closed_case(num_pes, n, driver_lengths)
    with defined(gpu, num_pes, XC.closed_tables(num_pes, n)[table]) as model:
        out = gpu.mqcl_evolve(num_pes, model, x, p, start, XC.MASS, length_x, length_p, XC.CLOSED_DT, XC.CLOSED_STEPS)
    err = XC.rel(out, expected)
    print(f"closed form num_pes {num_pes} n {n} driver lengths {driver_lengths} table {table}: err / tol {err / XC.CLOSED_TOL:.3g}, "
          f"moved {XC.rel(start, expected):.3g}")
    assert err <= XC.CLOSED_TOL
    assert np.array_equal(out, np.conj(np.swapaxes(out, 0, 1)))
    for a in range(num_pes):
        assert (out[a, a].imag == 0.0).all()


# ---- 2 - 4. DVR against MQCLE ----------------------------------------------------------------------------------------------------------------
_solved = {}


def solve(gpu, name, boundary):
    """one coupled case through both solvers, once per module: the DVR chain on `boundary`, the MQCLE from the device Wigner transform of
    psi0 (so the element conventions are shared by construction) at dt = 0.02 and 0.01, and the observables of both sides"""
    if (name, boundary) in _solved:
        return _solved[name, boundary]
    c = XC.COUPLED[name]
    num_pes, x, p, dx, dp, table = XC.coupled_case(name)
    n = len(x)
    psi0 = XC.packet(num_pes, x)
    with defined(gpu, num_pes, table) as model:
        H, E, basis = gpu.dvr_hamiltonian(num_pes, model, boundary, x[0], dx, n, XC.dvr_mass(boundary, n))
        lam, U = np.linalg.eigh(H)
        times = np.array([0.0, XC.T_END])
        psi = gpu.dvr_propagate(num_pes, n, U, lam, psi0, times)
        psi_adia = gpu.dvr_propagate(num_pes, n, U, lam, psi0, times, basis=basis)
        sums = XC.wigner_sum(c, boundary)
        W, _ = gpu.wigner(num_pes, sums, x[0], dx, p, psi)
        _, averages = gpu.wigner(num_pes, sums, x[0], dx, p, psi[1], energies=XC.diabatic_energies(table[2]), mass=XC.MASS, phase=False, averages=True)
        averages[0, 0] += XC.coupling_energy(W[1], table[2], dx, dp)
        energy = np.vdot(psi[1], H @ psi[1]).real * dx
        lengths = (n * dx, n * dp)
        rho = {dt: gpu.mqcl_evolve(num_pes, model, x, p, W[0], XC.MASS, *lengths, dt, int(round(XC.T_END / dt))) for dt in (XC.DT_COARSE, XC.DT_FINE)}
        combined = XC.richardson(rho[XC.DT_COARSE], rho[XC.DT_FINE])
        _, observed, populations = gpu.mqcl_observe(num_pes, model, x, p, combined, XC.MASS, dx, dp, adiabatic=False)
        quirk = None
        if name == "two-128" and boundary == XC.REFLECTIVE:  # the driver's lengths, n - 1 spacings
            quirk = gpu.mqcl_evolve(num_pes, model, x, p, W[0], XC.MASS, (n - 1) * dx, (n - 1) * dp, XC.DT_FINE, int(round(XC.T_END / XC.DT_FINE)))
    s = dict(case=c, x=x, p=p, dx=dx, dp=dp, energies=E, start=W[0], dvr=W[1], rho=rho, combined=combined, quirk=quirk,
             dvr_averages=averages[0], dvr_energy=energy, dvr_populations=XC.adiabatic_populations(psi_adia[1], num_pes, dx), observed=observed, populations=populations)
    s["err"] = {dt: XC.rel(rho[dt], W[1]) for dt in rho}
    s["err_combined"] = XC.rel(combined, W[1])
    _solved[name, boundary] = s
    return s


CHAINS = [(name, boundary) for name in ("two-128", "two-96", "three-128", "two-300") for boundary in (XC.REFLECTIVE, XC.PERIODIC)]
chains = pytest.mark.parametrize("name, boundary", CHAINS, ids=[f"{name}-{'periodic' if b else 'reflective'}" for name, b in CHAINS])


@chains
def test_mqcl_against_dvr(gpu, name, boundary):
    s = solve(gpu, name, boundary)
    c = s["case"]
    coarse, fine, both = s["err"][XC.DT_COARSE], s["err"][XC.DT_FINE], s["err_combined"]
    host = XC.host_richardson(c, boundary)
    print(f"{name} boundary {boundary}: dt 0.02 {coarse:.4e}, dt 0.01 {fine:.4e}, ratio {coarse / fine:.4f}, Richardson {both:.3e} "
          f"({both / host:.3g} of the host figure), the state moved {XC.rel(s['start'], s['dvr']):.3g}")
    assert XC.RATIO[0] <= coarse / fine <= XC.RATIO[1]                      # (a) second order, so the difference is the splitting's
    assert both <= XC.GPU_RICHARDSON * host                                # (b) and what is left once it is removed
    assert fine <= XC.GPU_PLAIN * c["plain"]                               # (c) a deterministic truncation error
    for out in s["rho"].values():
        assert np.array_equal(out, np.conj(np.swapaxes(out, 0, 1)))
        for a in range(c["num_pes"]):
            assert (out[a, a].imag == 0.0).all()


@chains
def test_observables_against_dvr(gpu, name, boundary):
    """gple_mqcl_observe of the Richardson-combined state: adiabatic populations against sum |psi_adia|^2 dx of gple_dvr_propagate(basis=),
    (E, x, p) against the averages of gple_wigner on the diabatic amplitudes (with the coupling term those averages leave out of E:
    exact_cases.coupling_energy) and E against psi^T H psi dx as well; each at the tolerance of (b) times the scale of its quantity
    (exact_cases.scales)"""
    s = solve(gpu, name, boundary)
    c = s["case"]
    tol = XC.GPU_RICHARDSON * XC.host_richardson(c, boundary)
    scale = XC.scales(s["dvr"], s["energies"], s["x"], s["p"], XC.MASS, s["dx"], s["dp"])
    d_pop = np.abs(s["populations"] - s["dvr_populations"])
    d_av = np.abs(s["observed"] - s["dvr_averages"])
    print(f"{name} boundary {boundary}: populations {s['populations']} off by {d_pop.max() / tol:.3g} tol; (E, x, p) {s['observed']} "
          f"off by {(d_av / scale).max() / tol:.3g} tol")
    assert (d_pop <= tol).all()
    assert (d_av <= tol * scale).all()
    assert abs(s["observed"][0] - s["dvr_energy"]) <= tol * scale[0]
    assert abs(s["populations"].sum() - 1.0) <= tol


def test_driver_lengths_are_visible(gpu):
    """quirk 1 of §12: with lengths of n - 1 spacings every shift is scaled by n / (n - 1), and the dt = 0.01 state sits more than 100 (c)
    bounds from the DVR answer: the comparison sees a relative error of 1 / n in a shift"""
    s = solve(gpu, "two-128", XC.REFLECTIVE)
    err = XC.rel(s["quirk"], s["dvr"])
    bound = XC.GPU_PLAIN * s["case"]["plain"]
    print(f"driver lengths at n = 128: {err:.3e} from the DVR answer, {err / bound:.3g} (c) bounds; n spacings: {s['err'][XC.DT_FINE]:.3e}")
    assert err > XC.QUIRK_FACTOR * bound
    assert s["err"][XC.DT_FINE] <= bound
