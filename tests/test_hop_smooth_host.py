"""CPU: the numpy restatement of gple_hop_smooth / gple_hop_smooth_mf (tests/hop_smooth_numpy.py), which the GPU tests lean on, against what the
definition implies (one trajectory, the normalisation and the first moments, the conjugate planes, the selection), the condition on the inputs
of the GPU test (the float64 restatement inside the bound B of the long double one in every case), the driver
hopping.run(phase_smooth=...) on a numpy stand-in api, and the new symbols of the built library.  The symbol test and the driver tests fail
without the feature."""
import os
import re

import numpy as np
import pytest

import gaussian_process_liouville_equation_amd as pkg
from gaussian_process_liouville_equation_amd import _capi, hopping, reconstruct
from tests import hop_density_mf_numpy as HDM
from tests import hop_numpy as HN
from tests import hop_outgoing_cases as HOC
from tests import hop_smooth_cases as SC
from tests import hop_smooth_numpy as HS
from tests.conftest import ROOT

RUN = dict(model=hopping.DAC, num_pes=2, ln_energy=-2.0, n_traj=48, seed=4, dt=4.0, x0=-4.0, xmin=-6.0, xmax=6.0)


def bits(a):
    return np.ascontiguousarray(a).view(np.float64).view(np.uint64)


def test_the_library_exports_and_the_binding_declares_the_smoothed_density():
    lib = pkg.load_library()  # no HIP call at load time: works without a GPU
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gple.h")).read(), flags=re.S)
    for name in ("hop_smooth", "hop_smooth_mf"):
        assert re.search(r"\bint\s+gple_%s\s*\(" % name, text), name
        assert name in _capi.GPLE_SYMBOLS
        f = getattr(lib, "gple_" + name)
        assert f.argtypes is not None and len(f.argtypes) == len(_capi.SIGNATURES[name][1])
        assert hasattr(_capi.Api, name)
    assert len(_capi.SIGNATURES["hop_smooth_mf"][1]) == len(_capi.SIGNATURES["hop_smooth"][1]) - 1  # no surface
    assert _capi.TIMER_HOP_SMOOTH == 20 and re.search(r"GPLE_TIMER_HOP_SMOOTH\s*=\s*20\b", text)
    assert hasattr(lib, "gple_debug_hop_smooth_split")


def one(x, p, b, surface=0, status=0):
    return (np.array([x]), np.array([p]), np.array([b], dtype=np.complex128), np.array([surface], dtype=np.int32), np.array([status], dtype=np.int32))


def test_one_trajectory_on_a_grid_point_is_the_separable_gaussian():
    pot = HN.builtin(HN.DAC, 2)
    grid = (-3.0, 0.25, 9, 8.0, 0.5, 7)
    h = (0.4, 0.9)
    state = one(-3.0 + 0.25 * 5, 8.0 + 0.5 * 2, [0.6, 0.8j], surface=1)
    s = HS.scale(3, h)
    g = np.outer(np.exp(-0.5 * ((np.arange(9) - 5) * 0.25 / 0.4) ** 2), np.exp(-0.5 * ((np.arange(7) - 2) * 0.5 / 0.9) ** 2))
    c = HDM.HD.amplitudes(pot, state)[0]
    for mean_field in (False, True):
        rho, tallies = HS.smooth(pot, state, grid, h, 3, mean_field)
        assert tallies == (1, 0) and rho.shape == (2, 2, 9, 7)
        u = np.abs(c) ** 2 if mean_field else np.array([0.0, 1.0])
        for a in range(2):
            assert np.allclose(rho[a, a].real, s * u[a] * g, rtol=1e-14, atol=0) and rho[a, a, 5, 2].real == pytest.approx(s * u[a], rel=1e-15)
        assert np.allclose(rho[0, 1], s * c[0] * np.conj(c[1]) * g, rtol=1e-14, atol=0)
    assert s == 1.0 / (3.0 * (2.0 * np.pi) * 0.4 * 0.9)


@pytest.mark.parametrize("name", ["dac10-fssh", "tsac"])
@pytest.mark.parametrize("mean_field", [False, True])
def test_normalisation_and_first_moments(name, mean_field):
    """a grid that reaches 8 h beyond every point, h = 1.5 d: sum rho_aa dx dp = used_a / n_norm and the first moments, to 1e-12"""
    c = HOC.case_of(SC.ENSEMBLES[name][0])
    state = HOC.ensemble(*SC.ENSEMBLES[name])
    x, p = state[0], state[1]
    dx, dp = 0.11, 0.37
    h = (1.5 * dx, 1.5 * dp)
    n_x, n_p = int(np.ceil((x.max() - x.min() + 16 * h[0]) / dx)) + 1, int(np.ceil((p.max() - p.min() + 16 * h[1]) / dp)) + 1
    grid = (x.min() - 8 * h[0], dx, n_x, p.min() - 8 * h[1], dp, n_p)
    rho, (used, nonfinite) = HS.smooth(c["potential"], state, grid, h, SC.N_TRAJ, mean_field, True)
    assert (used, nonfinite) == (SC.N_TRAJ, 0)
    _, _, u, _, _ = HS.terms(c["potential"], state, mean_field, True)
    xk, pj = grid[0] + dx * np.arange(n_x), grid[3] + dp * np.arange(n_p)
    for a in range(c["N"]):
        plane = rho[a, a].real
        assert plane.sum() * dx * dp == pytest.approx(u[a].sum() / SC.N_TRAJ, rel=1e-12)
        assert (plane.sum(axis=1) * xk).sum() * dx * dp == pytest.approx((u[a] * x).sum() / SC.N_TRAJ, rel=1e-12)
        assert (plane.sum(axis=0) * pj).sum() * dx * dp == pytest.approx((u[a] * p).sum() / SC.N_TRAJ, rel=1e-12)
    if not mean_field:
        assert np.array_equal(u[:c["N"]].sum(axis=1), np.bincount(state[3], minlength=c["N"]))


@pytest.mark.parametrize("name", list(SC.ENSEMBLES))
def test_lower_planes_are_conjugates_and_the_diagonal_is_real(name):
    c = HOC.case_of(SC.ENSEMBLES[name][0])
    state = HOC.ensemble(*SC.ENSEMBLES[name])
    grid = SC.grid_over(state, 24, 40)
    N = c["N"]
    for mean_field, bin_all in SC.FORMS:
        rho, _ = HS.smooth(c["potential"], state, grid, (1.5 * grid[1], 1.5 * grid[4]), SC.N_TRAJ, mean_field, bin_all)
        for a in range(N):
            assert not bits(rho[a, a].imag).any() and (rho[a, a].real >= 0).all()  # +0, bit for bit
            for b in range(a + 1, N):
                assert np.array_equal(rho[b, a], np.conj(rho[a, b])) and np.abs(rho[a, b]).max() > 0
    empty = tuple(np.asarray(v)[:5] for v in state[:4]) + (np.full(5, 7, dtype=np.int32),)
    rho, tallies = HS.smooth(c["potential"], empty, grid, (1.0, 1.0), 5)
    assert tallies == (0, 0) and not bits(rho).any()  # every sum is 0: +0 in the lower planes too


def test_the_selection():
    pot = HN.builtin(HN.DAC, 2)
    nan, inf = float("nan"), float("inf")
    #          used   finished  status 7  surface -1  surface 2  NaN x  inf x  NaN p   -inf p  finished with NaN x
    x = np.array([0.1, 0.2, 0.3, 0.4, 0.5, nan, inf, 0.6, 0.7, nan])
    p = np.array([9.0, 9.5, 9.1, 9.2, 9.3, 9.4, 9.6, nan, -inf, 9.0])
    status = np.array([0, 2, 7, 0, 0, 0, 0, 0, 0, 1], dtype=np.int32)
    surface = np.array([0, 1, 0, -1, 2, 0, 1, 0, 1, 0], dtype=np.int32)
    b = np.tile(np.array([0.6, 0.8j]), (10, 1))
    state = (x, p, b, surface, status)
    grid, h = (0.0, 0.1, 8, 9.0, 0.1, 8), (0.15, 0.15)
    want = {(False, False): (1, 4, [0]), (False, True): (2, 5, [0, 1]), (True, False): (3, 4, [0, 3, 4]), (True, True): (4, 5, [0, 1, 3, 4])}
    for (mean_field, bin_all), (used, nonfinite, who) in want.items():
        rho, tallies = HS.smooth(pot, state, grid, h, 10, mean_field, bin_all)
        assert tallies == (used, nonfinite) and np.isfinite(rho.view(np.float64)).all()
        alone, _ = HS.smooth(pot, tuple(v[who] for v in state), grid, h, 10, mean_field, True)  # the used ones alone, all running or finished
        assert np.array_equal(bits(rho), bits(alone))
    assert list(np.flatnonzero(HS.selection(state, False, True)[1])) == [5, 6, 7, 8, 9]


@pytest.mark.parametrize("name", list(SC.ENSEMBLES))
def test_the_float64_restatement_stays_inside_the_bound_in_every_gpu_case(name):
    """the condition on the inputs of tests/test_gpu_hop_smooth.py: a float64 evaluation in another order than the device's is inside B too"""
    c = HOC.case_of(SC.ENSEMBLES[name][0])
    state = HOC.ensemble(*SC.ENSEMBLES[name])
    assert all((state[4] == s).any() for s in (0, 1, 2))
    worst = 0.0
    for label, grid, h in SC.configurations(state):
        for mean_field, bin_all in SC.FORMS:
            assert SC.signs_are_safe(c["potential"], state, mean_field, bin_all)
            rho, tallies = HS.smooth(c["potential"], state, grid, h, SC.N_TRAJ, mean_field, bin_all)
            worst = max(worst, SC.check(rho, tallies, ("host", name, label, mean_field, bin_all), c["potential"], state, grid, h, SC.N_TRAJ, mean_field, bin_all))
    print(f"hop smooth {name}: float64 in index order against long double, the worst error over bound is {worst:.3f}")
    assert worst > 0.0


# ---- the driver ----------------------------------------------------------------------------------------------------------------------------------
def test_without_phase_smooth_the_run_is_the_one_it_was(tmp_path):
    """phase_smooth=None on stand-ins that have no hop_smooth: the calls and the keys of the run as it was"""
    for density, api_of, calls in ((None, HDM.HD.NumpyHopDensityApi, ["observe", "bin", "density", "evolve"]),
                                   ("amplitude", HDM.NumpyHopDensityMfApi, ["observe", "bin_mf", "density_mf", "evolve"])):
        api = api_of()
        assert not hasattr(api, "hop_smooth") and not hasattr(api, "hop_smooth_mf")
        res = hopping.run(api, out_dir=str(tmp_path / str(density)), phase_grid=(12, 10), phase_density=density, phase_smooth=None, **RUN)
        n_out = len(res["records"])
        assert api.calls[0] == ("sample", 48) and api.calls[1] == ("adiabatic",)
        assert [c[0] for c in api.calls[2:]] == (calls * n_out)[:-1]
        assert "phase_smooth" not in res and not any("smoothed" in r or "nonfinite" in r for r in res["records"])
        again = hopping.run(api_of(), out_dir=str(tmp_path / "again"), phase_grid=(12, 10), phase_density=density, **RUN)
        assert set(again) == set(res) and [set(r) for r in again["records"]] == [set(r) for r in res["records"]]
        assert (tmp_path / "again" / "phase.txt").read_bytes() == (tmp_path / str(density) / "phase.txt").read_bytes()


@pytest.mark.parametrize("method,density", [("fssh", None), ("fssh", "mixed"), ("fssh", "amplitude"), ("ehrenfest", "amplitude")])
@pytest.mark.parametrize("smooth", ["scott", (0.3, 1.7)])
def test_driver_with_the_smoothed_density(tmp_path, method, density, smooth):
    api = HS.NumpyHopSmoothApi()
    res = hopping.run(api, out_dir=str(tmp_path / "out"), phase_grid=(12, 10), phase_density=density, phase_smooth=smooth, method=method, **RUN)
    n_out = len(res["records"])
    s = res["setup"]
    h = (s["sigma_x"] * 48.0 ** (-1.0 / 6.0), s["sigma_p"] * 48.0 ** (-1.0 / 6.0)) if smooth == "scott" else (0.3, 1.7)
    assert res["phase_smooth"] == h and all(isinstance(v, float) for v in res["phase_smooth"])
    amplitude, mean_field = density == "amplitude", method == "ehrenfest"
    observe, evolve = ("observe_mf", "evolve_mf") if mean_field else ("observe", "evolve")
    bin_, smooth_ = ("bin_mf", "smooth_mf") if amplitude else ("bin", "smooth")
    assert api.calls[0] == ("sample", 48) and api.calls[1] == ("adiabatic",)
    assert [c[0] for c in api.calls[2:]] == ([observe, bin_, smooth_, evolve] * n_out)[:-1]  # the added call per output, no hop_density
    x, p = (reconstruct.read_grid(tmp_path / "out" / name) for name in ("x.txt", "p.txt"))
    grid = hopping.phase_grid_of(HS.NumpyHopSmoothApi(), 2, hopping.DAC, s, (12, 10))
    blocks = list(reconstruct.phase_blocks(str(tmp_path / "out" / "phase.txt"), 2, 12, 10))
    assert len(blocks) == n_out > 3 and len(x) == 12 and len(p) == 10
    # the states of the run again, for the fields the files must hold
    replay = HS.NumpyHopSmoothApi()
    state = replay.hop_sample(2, hopping.DAC, 48, 4, s["x0"], s["p0"], s["sigma_x"], s["sigma_p"], 0)
    for k, (rec, block) in enumerate(zip(res["records"], blocks)):
        running = int(rec["n_status"][0] if mean_field else rec["counts"][hopping.RUNNING].sum())
        assert (rec["smoothed"], rec["nonfinite"]) == (running, 0) and rec["binned"] + rec["outside"] == running
        assert ("binned_weights" in rec) == amplitude and ("binned_counts" in rec) != amplitude
        want, _ = (replay.hop_smooth_mf if amplitude else replay.hop_smooth)(2, hopping.DAC, state, grid, h, 48)
        values, lines = reconstruct._parse_host(block)
        assert lines == 4
        got = values.view(np.complex128).reshape(2, 2, 12, 10)
        assert np.allclose(got.view(np.float64), want.view(np.float64), rtol=5.1e-6, atol=1e-300)  # "%g": six significant digits
        if k + 1 < n_out:
            if mean_field:
                state = replay.hop_evolve_mf(2, hopping.DAC, state, s["mass"], 4.0, res["output_step"], s["xmin"], s["xmax"])
            else:
                state = replay.hop_evolve(2, hopping.DAC, state, 4, s["mass"], 4.0, k * res["output_step"], res["output_step"], s["xmin"], s["xmax"])
    # no out_dir: the call is made all the same, for its tallies
    api2 = HS.NumpyHopSmoothApi()
    res2 = hopping.run(api2, phase_grid=(12, 10), phase_density=density, phase_smooth=smooth, method=method, max_outputs=2, **RUN)
    assert [c[0] for c in api2.calls] == ["sample", "adiabatic", observe, bin_, smooth_, evolve, observe, bin_, smooth_]
    assert [r["smoothed"] for r in res2["records"]] == [r["smoothed"] for r in res["records"][:2]]


def test_driver_refuses_before_any_call():
    grid = dict(phase_grid=(8, 8))
    nan, inf = float("nan"), float("inf")
    bad_values = ["silverman", "Scott", "", (1.0,), (1.0, 2.0, 3.0), (0.0, 1.0), (1.0, -1.0), (nan, 1.0), (1.0, inf), ("a", "b"), 1.0, True, (None, 1.0)]
    cases = [dict(phase_smooth=v, **grid) for v in bad_values]
    cases += [dict(phase_smooth="scott"), dict(phase_smooth=(1.0, 1.0))]                                                  # no phase_grid
    cases += [dict(method="sqc", phase_smooth="scott", **grid), dict(method="mash", phase_smooth="scott", **grid),       # no phase_grid for them
              dict(method="ehrenfest", phase_smooth="scott", **grid), dict(method="ehrenfest", phase_density="mixed", phase_smooth="scott", **grid)]
    for bad in cases:
        api = HS.NumpyHopSmoothApi()
        with pytest.raises(ValueError):
            hopping.run(api, **{**RUN, **bad})
        assert api.calls == [], bad
