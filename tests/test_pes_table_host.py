"""CPU: the tabulated user potential (gple_pes_define) without a GPU — the float64 restatement the GPU tests lean on
(tests/pes_table_numpy.py) against the analytic DAC and its sharp error bounds, the nodes and the linear continuation, pes.tabulate, the
three new symbols, and the MQCLE driver on the numpy stand-in api with a table.  Only the symbol test needs the feature: the others check
the oracle."""
import math

import numpy as np
import pytest

from gaussian_process_liouville_equation_amd import _capi, exact_mqcl as EM, output, pes, steploop
from tests import pes_table_numpy as PT
from tests.test_mqcl_host import KW, NumpyApi

USER = 16


@pytest.mark.parametrize("dx", [1 / 2, 1 / 4, 1 / 8, 1 / 16])
def test_restatement_meets_the_hermite_bounds_on_dac(dx):
    """value error <= dx^4 / 384 f4 and derivative error <= sqrt(3) / 216 dx^3 f4 with f4 = max |V''''| over DAC's entries; the bounds are
    sharp (measured / bound 0.90 - 0.998), so only a relative 1e-6 is allowed for rounding"""
    table = PT.dac_table(dx)
    x = np.linspace(-16.0, 16.0, 20001)
    V, F = table.diabatic(x)
    Va, dVa = PT.dac(x)
    value, deriv = np.abs(V - Va).max(), np.abs(-F - dVa).max()
    bound_v, bound_d = dx ** 4 / 384 * PT.DAC_F4, math.sqrt(3) / 216 * dx ** 3 * PT.DAC_F4
    print(f"dx = {dx}: value {value / bound_v:.4f} of its bound, derivative {deriv / bound_d:.4f}")
    assert value <= bound_v * (1 + 1e-6)
    assert deriv <= bound_d * (1 + 1e-6)
    assert value >= 0.5 * bound_v and deriv >= 0.5 * bound_d  # (sharp: a restatement that interpolated better than a cubic can would be wrong too)


def test_nodes_carry_their_own_bits():
    table = PT.random_table(3, 65, np.random.default_rng(5), x_first=-4.0, dx=0.125)  # dyadic: the nodes and s are exact
    V, F = table.diabatic(table.nodes()[:-1])
    assert np.array_equal(V, table.V[:-1])
    assert np.abs(-F - table.dV[:-1]).max() <= 4 * PT.EPS * np.abs(table.dV).max()


def test_last_node_and_linear_continuation():
    table = PT.random_table(2, 9, np.random.default_rng(6), x_first=-1.0, dx=0.25)
    last = table.nodes()[-1]
    # exactly at the last node: the interval n - 2 at t = 1, not the continuation
    s, k, t, left, right = table.locate(np.array([last]))
    assert k[0] == table.n - 2 and t[0] == 1.0 and not left[0] and not right[0]
    V, F = table.diabatic([last])
    assert np.abs(V[0] - table.V[-1]).max() <= table.tolerance([last]).max()
    assert np.abs(-F[0] - table.dV[-1]).max() <= table.tolerance([last]).max() / table.dx
    for x, node in ((-1.0 - 3.7, 0), (np.nextafter(-1.0, -2.0), 0), (last + 11.0, -1), (last + 2.0 ** -30, -1)):
        V, F = table.diabatic([x])
        assert np.array_equal(-F[0], table.dV[node])
        assert np.array_equal(V[0], table.V[node] + table.dV[node] * (x - table.nodes()[node]))
    # C^1 at both ends: value and slope of the two branches meet
    for x_in, x_out in ((-1.0, np.nextafter(-1.0, -2.0)), (last, last + 2.0 ** -30)):
        (Vi, Fi), (Vo, Fo) = table.diabatic([x_in]), table.diabatic([x_out])
        assert np.abs(Vi - Vo).max() <= 1e-10 and np.abs(Fi - Fo).max() <= 1e-10  # (2^-30 apart, slopes and curvatures below 0.1)


def test_two_node_table():
    table = PT.Table(0.5, 2.0, *PT.dac(np.array([0.5, 2.5])))
    x = np.array([0.5, 1.5, 2.5, -3.0, 7.0])
    V, F = table.diabatic(x)
    assert np.array_equal(V[0], table.V[0])
    # the midpoint of a cubic Hermite segment: (V0 + V1) / 2 + dx (V0' - V1') / 8
    mid = 0.5 * (table.V[0] + table.V[1]) + 2.0 * (table.dV[0] - table.dV[1]) / 8.0
    assert np.abs(V[1] - mid).max() <= 8 * PT.EPS * np.abs(table.V).max()
    assert np.abs(V[2] - table.V[1]).max() <= table.tolerance([2.5]).max()
    assert np.array_equal(V[3], table.V[0] + table.dV[0] * (-3.0 - 0.5)) and np.array_equal(V[4], table.V[1] + table.dV[1] * (7.0 - 2.5))


def test_tabulate():
    x_first, dx, V, dV = pes.tabulate(lambda x: PT.dac(x), -16.0, 1 / 16, 513)
    ref = PT.dac_table(1 / 16)
    assert (x_first, dx) == (-16.0, 1 / 16) and np.array_equal(V, ref.V) and np.array_equal(dV, ref.dV)
    # both triangles are made equal
    skew = lambda x: (np.array([[0.0, 1.0 + x], [1.0 + x + 1e-17, 0.5]]), np.array([[0.0, 1.0], [1.0, 0.0]]))
    _, _, V, dV = pes.tabulate(skew, 0.0, 0.5, 3)
    assert np.array_equal(V, np.swapaxes(V, 1, 2)) and V.shape == (3, 2, 2)
    for bad in (dict(n=1), dict(dx=0.0), dict(dx=float("nan")), dict(x_first=float("inf"))):
        kw = dict(x_first=0.0, dx=0.5, n=3)
        kw.update(bad)
        with pytest.raises(ValueError):
            pes.tabulate(skew, kw["x_first"], kw["dx"], kw["n"])
    with pytest.raises(ValueError):
        pes.tabulate(lambda x: (np.zeros((2, 3)), np.zeros((2, 3))), 0.0, 0.5, 3)
    with pytest.raises(ValueError):
        pes.tabulate(lambda x: (np.full((2, 2), np.inf), np.zeros((2, 2))), 0.0, 0.5, 3)


def test_new_symbols_are_exported_and_declared():
    """fails without the feature, needs no GPU"""
    import gaussian_process_liouville_equation_amd as pkg

    lib = pkg.load_library()
    for name, nargs in (("pes_define", 9), ("pes_undefine", 2), ("pes_diabatic_n", 8)):
        assert name in _capi.GPLE_SYMBOLS
        f = getattr(lib, "gple_" + name)
        assert f.argtypes is not None and len(f.argtypes) == nargs
    assert _capi.PES_USER == steploop.PES_USER == USER
    for method in ("pes_define", "pes_undefine", "pes_diabatic_n"):
        assert callable(getattr(_capi.Api, method))


def test_install_leaves_the_built_in_models_alone(monkeypatch):
    x = np.linspace(-3, 3, 7)
    before = PT.ON.adiabatic(x, 1, 3)
    table = PT.function_table(PT.three_level, -8.0, 8.0, 0.25)
    PT.install(monkeypatch, {USER: table})
    for a, b in zip(before, PT.ON.adiabatic(x, 1, 3)):
        assert np.array_equal(a, b)
    E, C, F, NAC = PT.ON.adiabatic(x, USER, 3)  # not the spectator branch of the oracle: every state is coupled
    V, Fd = table.diabatic(x)
    assert np.abs(np.einsum("mak,mk,mbk->mab", C, E, C) - V).max() <= 1e-15
    assert (np.abs(NAC[:, 2, 0]) > 0).all() and (np.diff(E, axis=1) > 0).all()


class StepApi:
    """records which tick entry point steploop takes"""

    def __init__(self):
        self.calls = []

    def evolve(self, fits, model, mass, dt, density, new_points=False):
        self.calls.append(("evolve", model))
        return density

    def evolve_n(self, num_pes, fits, model, mass, dt, density, new_points=False):
        self.calls.append(("evolve_n", num_pes, model))
        return density


class NoKernels:
    num_pes = 2

    def __call__(self, i, j=None):
        return None


def test_steploop_sends_a_user_model_through_the_n_level_tick():
    api = StepApi()
    dens = {(0, 0): (np.zeros((3, 2)), np.zeros(3, dtype=complex))}
    steploop.evolve(dens, 2000.0, 1.0, NoKernels(), steploop.DAC, api)
    steploop.evolve(dens, 2000.0, 1.0, NoKernels(), USER + 2, api)
    steploop.new_point_predict(np.zeros((2, 2)), 1, 0, 2000.0, 1.0, NoKernels(), USER, api)
    steploop.new_point_predict(np.zeros((2, 2)), 1, 0, 2000.0, 1.0, NoKernels(), steploop.ECR, api)
    assert api.calls == [("evolve", 1), ("evolve_n", 2, USER + 2), ("evolve_n", 2, USER), ("evolve", 2)]


def test_model_potential_goes_through_the_n_level_energies(monkeypatch):
    PT.install(monkeypatch, {USER: PT.function_table(PT.other_dac, -8.0, 8.0, 0.125)})
    x = np.linspace(-5, 5, 11)
    potential = output.model_potential(NumpyApi(), 2, USER)
    E = PT.ON.adiabatic(x, USER, 2)[0]
    assert np.array_equal(potential(x, 0), E[:, 0]) and np.array_equal(potential(x, 1), E[:, 1])


def test_mqcl_driver_runs_a_user_model_on_the_stand_in_api(monkeypatch, tmp_path):
    """exact_mqcl.run passes the id through unchanged, and final_line takes its else branch (p0) for a user model"""
    PT.install(monkeypatch, {USER: PT.function_table(PT.other_dac, -12.0, 12.0, 0.125)})
    res = EM.run(NumpyApi(), model=USER, num_pes=2, out_dir=str(tmp_path), write_phase=None, max_outputs=1, **KW)
    s = res["setup"]
    pops = EM.populations(res["rho"], s["dx"], s["dp"])
    assert res["final_line"] == " ".join("%g" % v for v in [s["p0"], *pops])
    assert len(res["records"]) == 2 and abs(sum(res["records"][1]["populations"]) - 1.0) <= 1e-6
    assert abs(res["records"][1]["populations"][1]) > 1e-5  # the table's coupling moved population


# ---- the DVR driver on its numpy stand-in (tests/test_dvr_absorbing_host.py) ---------------------------------------------------------------
def _dvr_table(num_pes):
    return PT.function_table(PT.other_dac if num_pes == 2 else PT.three_level, -8.0, 8.0, 0.125)


@pytest.mark.parametrize("num_pes", [2, 3])
def test_absorbing_dvr_driver_runs_a_user_model_on_the_stand_in_api(monkeypatch, tmp_path, num_pes):
    """exact.run(boundary=ABSORBING) with a user id against the restated absorbing loop with the table's Hamiltonian and bases: the absorbing
    boundary takes its H from gple_dvr_hamiltonian like the other two, so a user model reaches it through the same id"""
    from gaussian_process_liouville_equation_amd import exact
    from tests import dvr_absorbing_numpy as AN
    from tests.test_dvr_absorbing_host import SMALL, NumpyApi as DvrApi

    PT.install(monkeypatch, {USER: _dvr_table(num_pes)})
    api = DvrApi()
    res = exact.run(api, model=USER, num_pes=num_pes, boundary=exact.ABSORBING, out_dir=str(tmp_path), write_phase=None, max_outputs=4, **SMALL)
    s = res["setup"]
    assert [c for c in api.calls if c[0] == "hamiltonian"] == [("hamiltonian", 0)]
    ref, _ = AN.run_loop(s, num_pes, USER, 4, PT.ON.adiabatic(s["x"], USER, num_pes)[1])
    assert len(res["records"]) == len(ref) == 4
    for a, b in zip(res["records"], ref):
        assert a["t"] == b["t"]
        assert np.abs(a["populations"] - b["populations"]).max() <= 1e-12
        assert abs(a["E"] - b["E"]) <= 1e-12 * abs(b["E"]) and abs(a["x"] - b["x"]) <= 1e-12
    # the table's couplings act: population has reached the upper surfaces, and a run on the built-in SAC differs
    assert res["records"][-1]["populations"][1] > 1e-6
    sac = exact.run(DvrApi(), model=exact.SAC, num_pes=num_pes, boundary=exact.ABSORBING, write_phase=None, max_outputs=4, **SMALL)
    assert np.abs(sac["records"][-1]["populations"] - res["records"][-1]["populations"]).max() > 1e-6
    rows = open(tmp_path / "averages.txt").read().splitlines()
    assert len(rows) == 4 and [float(v) for v in rows[3].split()][4:4 + num_pes] == [float("%g" % v) for v in ref[3]["populations"]]
    line = res["final_line"].split()
    assert len(line) == 1 + num_pes and line[0] == "%g" % s["p0"]  # a user model: p0, the else branch


@pytest.mark.parametrize("boundary", [0, 1])
def test_spectral_dvr_driver_runs_a_user_model_on_the_stand_in_api(monkeypatch, boundary):
    """the reflective and the periodic run on the stand-in with a spectral propagation of its own, against tests/dvr_numpy.run_loop"""
    from gaussian_process_liouville_equation_amd import exact
    from tests import dvr_numpy as DN
    from tests.test_dvr_absorbing_host import SMALL, NumpyApi as DvrApi

    class Spectral(DvrApi):
        def dvr_propagate(self, num_pes, n, eigvec, eigval, psi0, times):
            c0 = eigvec.T @ psi0
            return np.stack([eigvec @ (np.exp(-1j * eigval * t / DN.HBAR) * c0) for t in times])

    PT.install(monkeypatch, {USER: _dvr_table(2)})
    api = Spectral()
    res = exact.run(api, model=USER, num_pes=2, boundary=boundary, write_phase=None, max_outputs=4, **SMALL)
    s = res["setup"]
    E, C, _, _ = PT.ON.adiabatic(s["x"], USER, 2)
    ref = DN.run_loop(2, USER, boundary, s, 4, (E, C))
    assert ("hamiltonian", boundary) in api.calls and len(res["records"]) == len(ref)
    for a, b in zip(res["records"], ref):
        assert a["t"] == b["t"]
        assert np.abs(a["populations"] - b["populations"]).max() <= 1e-12
        for k in ("E", "x", "p"):
            assert abs(a[k] - b[k]) <= 1e-12 * max(1.0, abs(b[k])), (k, a[k], b[k])
        assert (np.abs(a["phase_averages"] - b["phase_averages"]) <= 1e-12 * np.maximum(1.0, np.abs(b["phase_averages"]))).all()
    assert res["final_line"].split()[0] == "%g" % s["p0"]
