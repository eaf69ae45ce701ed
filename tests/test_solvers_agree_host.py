"""CPU: the claims that tests/test_gpu_solvers_agree.py rests on, on the numpy restatements (tests/mqcl_numpy.py, tests/dvr_numpy.py,
tests/pes_table_numpy.py) — on V = k x^2 / 2 I + A + B x the MQCLE density and the partial Wigner transform of the DVR wavefunction differ by
the Strang splitting alone (second order, removed by Richardson), and with B = 0 and diagonal A the MQCLE steps follow a closed form
(DESIGN.md §12).  The figures asserted here are the reference's numbers from which the GPU tolerances are set (tests/exact_cases.py), and
the conditions of every case (the state away from the box edges, the p grid inside the Wigner alias limit) are asserted here, not measured."""
import math

import numpy as np
import pytest

from tests import dvr_numpy as DN
from tests import exact_cases as XC
from tests import mqcl_numpy as MN
from tests import pes_table_numpy as PT

MODEL = 16  # any id the oracle does not know: the restatements see the table under it


@pytest.fixture
def install(monkeypatch):
    tables = {}
    PT.install(monkeypatch, tables)

    def make(table):
        tables[MODEL] = PT.Table(*table)
        return MODEL

    return make


# ---- the helper's own closed forms ------------------------------------------------------------------------------------------------------------
def test_strang_map_and_closed_form_basics():
    M = XC.strang_map(0.05, 1.0, 1.0, 1.0)
    assert abs(np.linalg.det(M) - 1.0) <= 1e-15
    # one step of the oscillator to second order: the rotation by dt up to dt^3
    assert np.abs(M - np.array([[math.cos(0.05), math.sin(0.05)], [-math.sin(0.05), math.cos(0.05)]])).max() <= 0.05 ** 3 / 4
    # the literal product, scaled
    f = 128 / 127
    D, K = np.array([[1.0, f * 0.025 / 2.0], [0.0, 1.0]]), np.array([[1.0, 0.0], [-f * 3.0 * 0.05, 1.0]])
    assert np.array_equal(XC.strang_map(0.05, 2.0, 3.0, f), D @ K @ D)
    x, _ = XC.box(32, 16.0)
    gaps = XC.gaps_of(XC.CLOSED_A[3])
    assert gaps[0, 1] == 0.7 and gaps[1, 2] == 1.8 and np.array_equal(gaps, -gaps.T)
    start = XC.closed_form(x, x, 2.0, 0.5, 0.6, M, 0, gaps, 0.0, XC.CLOSED_W[3])
    assert np.array_equal(start, XC.CLOSED_W[3][:, :, None, None] * XC.wigner_gauss(x, x, 2.0, 0.5, 0.6)[None, None])
    assert np.array_equal(XC.CLOSED_W[3], np.conj(XC.CLOSED_W[3].T)) and np.array_equal(XC.CLOSED_W[2], np.conj(XC.CLOSED_W[2].T))
    # a quarter period of the exact flow carries (x0, p0) to (p0, -x0): the map's K-th power does, up to its second-order phase error
    q = np.linalg.matrix_power(XC.strang_map(math.pi / 2 / 400, 1.0, 1.0, 1.0), 400) @ np.array([2.0, 0.5])
    assert np.abs(q - np.array([0.5, -2.0])).max() <= 1e-5


@pytest.mark.parametrize("num_pes", [2, 3])
def test_both_tables_are_the_quadratic(num_pes):
    """a cubic Hermite segment reproduces a quadratic: on the grid and between the nodes of the coarse, offset table, value and force"""
    x, dx = XC.box(127, XC.CLOSED_GRIDS[127][0])
    assert XC.closed_tables(num_pes, 127)["coarse"][1] == 0.5
    for name, table in XC.closed_tables(num_pes, 127).items():
        t = PT.Table(*table)
        nodes = t.nodes()
        assert nodes[0] <= x[0] and nodes[-1] >= x[-1]  # no linear continuation on the grid
        if name == "coarse":
            assert np.abs((x[:, None] - nodes[None, :])).min() > 1e-3  # no node on the grid
        V, F = t.diabatic(x)
        Vq, dVq = XC.quadratic_table(num_pes, XC.K_FORCE, XC.CLOSED_A[num_pes], np.zeros((num_pes, num_pes)), x[0], dx, len(x))
        assert np.abs(V - Vq).max() <= 64 * PT.EPS * np.abs(Vq).max() and np.abs(-F - dVq).max() <= 64 * PT.EPS * np.abs(Vq).max() / t.dx


# ---- the closed form against the restatement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_pes, n, driver_lengths, table", [(2, 64, False, "grid"), (2, 64, False, "coarse"), (2, 64, True, "grid"),
                                                                (2, 64, True, "coarse"), (3, 64, True, "grid"), (2, 127, False, "grid")])
def test_closed_form_holds_on_the_restatement(install, num_pes, n, driver_lengths, table):
    """measured over every GPU case (five sizes, both lengths, both tables, two and three levels): 6.5e-15 ... 2.7e-14 of max |rho|, against
    the 2e-13 allowed; the subset here is what fits the file's time (n = 64 is the tight grid, 127 the largest figure)"""
    x, p, (length_x, length_p), f, start, expected = XC.closed_case(num_pes, n, driver_lengths)
    model = install(XC.closed_tables(num_pes, n)[table])
    out = MN.evolve(start, MN.Bases(x, model, num_pes), p, XC.MASS, length_x, length_p, XC.CLOSED_DT, XC.CLOSED_STEPS)
    err = XC.rel(out, expected)
    print(f"closed form num_pes {num_pes} n {n} f {f:.5f} table {table}: {err:.3e} of max |rho| ({err / XC.CLOSED_HOST:.3g} of the allowance)")
    assert err <= XC.CLOSED_HOST
    assert XC.rel(start, expected) > 0.5  # the packet has gone elsewhere
    if driver_lengths:  # and the scaling of the shears is no detail: the unscaled map is far off
        plain = XC.closed_form(x, p, XC.CLOSED_X0, XC.CLOSED_P0, XC.CLOSED_GRIDS[n][1], XC.strang_map(XC.CLOSED_DT, XC.MASS, XC.K_FORCE, 1.0),
                               XC.CLOSED_STEPS, XC.gaps_of(XC.CLOSED_A[num_pes]), XC.CLOSED_STEPS * XC.CLOSED_DT, XC.CLOSED_W[num_pes])
        assert XC.rel(out, plain) > 1e-3


# ---- DVR against MQCLE ----------------------------------------------------------------------------------------------------------------------------
def dvr_side(install, name, boundary):
    """the DVR chain of one case on the restatements: (W0, W(T), psi_adia(T), energies, model, grids)"""
    c = XC.COUPLED[name]
    num_pes, x, p, dx, dp, table = XC.coupled_case(name)
    n = len(x)
    model = install(table)
    H = DN.hamiltonian(num_pes, model, boundary, x[0], dx, n, XC.dvr_mass(boundary, n))
    lam, U = np.linalg.eigh(H)
    psi0 = XC.packet(num_pes, x)
    psi = U @ (np.exp(-1j * lam * XC.T_END) * (U.T @ psi0))
    sums = XC.wigner_sum(c, boundary)
    W0, _ = DN.wigner(psi0, num_pes, sums, dx, p, dtype=np.complex128)
    W, _ = DN.wigner(psi, num_pes, sums, dx, p, dtype=np.complex128)
    return dict(case=c, num_pes=num_pes, x=x, p=p, dx=dx, dp=dp, n=n, model=model, table=table, H=H, start=W0, dvr=W, psi=psi)


@pytest.mark.parametrize("boundary", [XC.REFLECTIVE, XC.PERIODIC])
@pytest.mark.parametrize("name", sorted(XC.COUPLED))
def test_conditions_of_every_case(install, name, boundary):
    s = dvr_side(install, name, boundary)
    edge0, edge = XC.edge_fraction(s["start"]), XC.edge_fraction(s["dvr"])
    print(f"{name} boundary {boundary}: edge {edge0:.2e} at t = 0, {edge:.2e} at T; max |p| {np.abs(s['p']).max():.3g} of {math.pi / 2 / s['dx']:.4g}")
    assert edge0 <= XC.EDGE and edge <= XC.EDGE
    assert np.abs(s["p"]).max() < math.pi / (2.0 * s["dx"])
    # the runs are not trivial: every diabat is populated and the coherence is of the size of the populations
    n, num_pes = s["n"], s["num_pes"]
    pops = np.array([(np.abs(s["psi"][a * n:(a + 1) * n]) ** 2).sum() * s["dx"] for a in range(num_pes)])
    assert pops.min() > 0.15 and abs(pops.sum() - 1.0) <= 1e-12
    diag = max(np.abs(s["dvr"][a, a]).max() for a in range(num_pes))
    assert max(np.abs(s["dvr"][a, b]).max() for a in range(num_pes) for b in range(a + 1, num_pes)) > 0.5 * diag
    if num_pes == 2:
        assert np.abs(pops - np.array([0.314, 0.686])).max() <= 1e-3
    else:
        assert np.abs(pops - np.array([0.386, 0.447, 0.166])).max() <= 1e-3


def test_wide_box_takes_the_periodic_wigner_sum(install):
    """on the box of 30 the periodic sum is the sum without wrap-around; on a box of 16 it is not (exact_cases.wigner_sum)"""
    s = dvr_side(install, "two-300", XC.REFLECTIVE)
    Wp, _ = DN.wigner(s["psi"], 2, XC.PERIODIC, s["dx"], s["p"], dtype=np.complex128)
    assert XC.rel(Wp, s["dvr"]) <= XC.EDGE
    assert XC.wigner_sum(XC.COUPLED["two-300"], XC.PERIODIC) == XC.PERIODIC
    s = dvr_side(install, "two-96", XC.REFLECTIVE)
    Wp, _ = DN.wigner(s["psi"], 2, XC.PERIODIC, s["dx"], s["p"], dtype=np.complex128)
    assert XC.rel(Wp, s["dvr"]) > 1e-3
    assert XC.wigner_sum(XC.COUPLED["two-96"], XC.PERIODIC) == XC.REFLECTIVE


def test_periodic_kinetic_matrix_carries_the_length_of_n_minus_1_spacings():
    """exact_cases.dvr_mass: the periodic kinetic block is the Fourier matrix of period n dx (eigenvalues (2 pi j / (n dx))^2 / 2m, odd n)
    once the mass is scaled by (n / (n - 1))^2"""
    n, dx = 33, 0.25
    T = DN.hamiltonian(2, 0, DN.PERIODIC, -4.0, dx, n, XC.dvr_mass(XC.PERIODIC, n))[:n, :n]
    V = np.diag(np.diag(DN.hamiltonian(2, 0, DN.PERIODIC, -4.0, dx, n, 1e300)[:n, :n]))  # (the potential alone: no kinetic energy at this mass)
    j = np.arange(-(n // 2), n // 2 + 1)
    assert np.abs(np.linalg.eigvalsh(T - V) - np.sort((2 * math.pi * j / (n * dx)) ** 2 / 2.0)).max() <= 1e-11 * (math.pi / dx) ** 2


def mqcl_side(s, dts, lengths=None):
    n, dx, dp = s["n"], s["dx"], s["dp"]
    bases = MN.Bases(s["x"], s["model"], s["num_pes"])
    lengths = (n * dx, n * dp) if lengths is None else lengths
    return bases, {dt: MN.evolve(s["start"], bases, s["p"], XC.MASS, *lengths, dt, int(round(XC.T_END / dt))) for dt in dts}


def check_observables(s, bases, combined, tol):
    """MN.observe of the Richardson state against the DVR side: adiabatic populations from psi, (E, x, p) from the averages of the Wigner
    function of the diabatic amplitudes (exact_cases.coupling_energy adds what those averages leave out of E)"""
    num_pes, n = s["num_pes"], s["n"]
    _, av, pops = MN.observe(combined, bases, s["x"], s["p"], XC.MASS, s["dx"], s["dp"])
    psi_adia = np.einsum("ajk,ja->ka", bases.C, s["psi"].reshape(num_pes, n)).reshape(-1)
    V = s["table"][2]
    ref = DN.wigner_averages(s["dvr"], s["x"], s["p"], XC.diabatic_energies(V), XC.MASS, s["dx"])
    ref[0] += XC.coupling_energy(s["dvr"], V, s["dx"], s["dp"])
    # the energy of the wavefunction itself, and why the transform is taken of the diabatic amplitudes: the Wigner transform of the
    # adiabatic ones is another function where the adiabatic states turn with x, and its averages lie percents away
    assert abs(ref[0] - np.vdot(s["psi"], s["H"] @ s["psi"]).real * s["dx"]) <= 1e-12 * abs(ref[0])
    W_adia, _ = DN.wigner(psi_adia, num_pes, XC.REFLECTIVE, s["dx"], s["p"], dtype=np.complex128)
    assert abs(DN.wigner_averages(W_adia, s["x"], s["p"], bases.E, XC.MASS, s["dx"])[2] - ref[2]) > 1e-2
    scale = XC.scales(s["dvr"], bases.E, s["x"], s["p"], XC.MASS, s["dx"], s["dp"])
    d_pop, d_av = np.abs(pops - XC.adiabatic_populations(psi_adia, num_pes, s["dx"])), np.abs(av - ref)
    print(f"   populations {pops} off by {d_pop.max() / tol:.3g} tol; (E, x, p) {av}, scales {scale}, off by {(d_av / scale).max() / tol:.3g} tol")
    assert (d_pop <= tol).all() and (d_av <= tol * scale).all()


def test_second_order_and_richardson_at_96(install):
    """three time steps, so two ratios; both DVR boundaries share the MQCLE runs (the start is the same sum on this box)"""
    s = dvr_side(install, "two-96", XC.REFLECTIVE)
    bases, rho = mqcl_side(s, (0.04, 0.02, 0.01))
    for boundary in (XC.REFLECTIVE, XC.PERIODIC):
        d = s if boundary == XC.REFLECTIVE else dvr_side(install, "two-96", boundary)
        assert np.array_equal(d["start"], s["start"])
        err = {dt: XC.rel(out, d["dvr"]) for dt, out in rho.items()}
        combined = XC.richardson(rho[0.02], rho[0.01])
        both = XC.rel(combined, d["dvr"])
        print(f"two-96 boundary {boundary}: {err[0.04]:.4e} {err[0.02]:.4e} {err[0.01]:.4e}, ratios {err[0.04] / err[0.02]:.4f} "
              f"{err[0.02] / err[0.01]:.4f}, Richardson {both:.3e}")
        assert XC.RATIO[0] <= err[0.04] / err[0.02] <= XC.RATIO[1] and XC.RATIO[0] <= err[0.02] / err[0.01] <= XC.RATIO[1]
        assert both <= XC.host_richardson(d["case"], boundary)
        assert err[0.01] <= d["case"]["plain"]
        assert both < err[0.01] / 1000  # fourth order left: the second-order term was all there was
        check_observables(d, bases, combined, XC.host_richardson(d["case"], boundary))


def test_figures_at_128(install):
    """the two-level case of the table of §12 at n = 128: the figures of (b) and (c)"""
    s = dvr_side(install, "two-128", XC.REFLECTIVE)
    _, rho = mqcl_side(s, (XC.DT_COARSE, XC.DT_FINE))
    for boundary in (XC.REFLECTIVE, XC.PERIODIC):
        d = s if boundary == XC.REFLECTIVE else dvr_side(install, "two-128", boundary)
        err = {dt: XC.rel(out, d["dvr"]) for dt, out in rho.items()}
        both = XC.rel(XC.richardson(rho[XC.DT_COARSE], rho[XC.DT_FINE]), d["dvr"])
        print(f"two-128 boundary {boundary}: {err[XC.DT_COARSE]:.4e} {err[XC.DT_FINE]:.4e}, ratio {err[XC.DT_COARSE] / err[XC.DT_FINE]:.4f}, Richardson {both:.3e}")
        assert XC.RATIO[0] <= err[XC.DT_COARSE] / err[XC.DT_FINE] <= XC.RATIO[1]
        assert both <= XC.host_richardson(d["case"], boundary)
        assert err[XC.DT_FINE] <= d["case"]["plain"]
        # the margins of the GPU test leave the figure visible: the bound of (c) is below the error at the coarser step
        assert XC.GPU_PLAIN * d["case"]["plain"] < err[XC.DT_COARSE] / 2


def test_recorded_figures_are_consistent():
    """the recorded rows (three levels, n = 300) were measured once with the code above: what can be checked of them without the runs"""
    for name, c in XC.COUPLED.items():
        assert 3.4e-5 < c["plain"] < 4.0e-5 and all(6e-9 < r < 1.3e-8 for r in c["richardson"])
        # the quirk test needs its factor of 100 to be a statement about 1 / n: 100 (c) bounds lie below the 1 / n shift error of 2.9e-2
        assert XC.QUIRK_FACTOR * XC.GPU_PLAIN * c["plain"] < 2.9e-2 / 5
