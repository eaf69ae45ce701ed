"""CPU: the numpy restatement of gple_hop_bin_mf / gple_hop_density_mf (tests/hop_density_mf_numpy.py), which the GPU tests lean on, against the
restatements it has to agree with (the mixed density of tests/hop_density_numpy.py, the sums of tests/hop_mf_numpy.py), the driver
hopping.run(phase_grid=..., phase_density=...) on a numpy stand-in api, and the new symbols of the built library.  The symbol test and the
driver tests fail without the feature.

The ensembles: 293 trajectories, seed 0, x0 = -4, sigma_p = p0 / 20, bounds +-6, mass 2000; DAC at p0 = 16 (dt = 1, 250 steps: all running), DAC
at p0 = 10 (dt = 2, 900 steps: all three statuses) and TSAC from the middle surface (dt = 4, 400 steps), evolved by hop_mf_numpy.evolve."""
import functools
import math
import os
import re

import numpy as np
import pytest

import gaussian_process_liouville_equation_amd as pkg
from gaussian_process_liouville_equation_amd import _capi, hopping, reconstruct
from tests import hop_density_mf_numpy as HDM
from tests import hop_density_numpy as HD
from tests import hop_mf_numpy as HM
from tests import hop_numpy as HN
from tests.conftest import ROOT

EPS = np.finfo(np.float64).eps
N_TRAJ, MASS, SEED, X0, LEFT, RIGHT = 293, 2000.0, 0, -4.0, -6.0, 6.0
TWO32 = 4294967296
CASES = {"dac16": (HN.DAC, 2, 16.0, 1.0, 250, 0), "dac10": (HN.DAC, 2, 10.0, 2.0, 900, 0), "tsac": (HN.TSAC, 3, 10.0, 4.0, 400, 1)}
RUN = dict(model=hopping.DAC, num_pes=2, ln_energy=-2.0, n_traj=48, seed=4, dt=4.0, x0=-4.0, xmin=-6.0, xmax=6.0)


@functools.lru_cache(maxsize=None)
def ensemble(name):
    """(potential, N, the fresh sample, the sample after the mean-field steps)"""
    model, N, p0, dt, steps, surface0 = CASES[name]
    pot = HN.builtin(model, N)
    start = HN.sample(pot, N, N_TRAJ, SEED, X0, p0, 1.0 / (2.0 * p0 / 20.0), p0 / 20.0, surface0=surface0)
    end, _ = HM.evolve(pot, start, MASS, dt, steps, LEFT, RIGHT)
    return pot, N, start, end


def grids(state):
    """16 x 9 over the bounds and the momenta, the same with a fifth of the momentum range cut off at either end, 1 x 1 over everything"""
    p = state[1]
    out = []
    for margin in (0.0, 0.2):
        lo, hi = p.min() + margin * (p.max() - p.min()), p.max() - margin * (p.max() - p.min())
        out.append((LEFT, 12.0 / 15.0, 16, lo, max(hi - lo, 1.0) / 8.0, 9))
    return out + [(0.0, 1e3, 1, 0.0, 1e3, 1)]


def split(acc, N, grid):
    n_cells = grid[2] * grid[5]
    return acc[:N * n_cells].reshape(N, n_cells), acc[N * n_cells:-2].reshape(N * (N - 1), n_cells), acc[-2:]


def test_the_library_exports_and_the_binding_declares_the_amplitude_density_entry_points():
    lib = pkg.load_library()  # no HIP call at load time: works without a GPU
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gple.h")).read(), flags=re.S)
    for name in ("hop_bin_mf", "hop_density_mf"):
        assert re.search(r"\bint\s+gple_%s\s*\(" % name, text), name
        assert name in _capi.GPLE_SYMBOLS
        f = getattr(lib, "gple_" + name)
        assert f.argtypes is not None and len(f.argtypes) == len(_capi.SIGNATURES[name][1])
        assert hasattr(_capi.Api, name)
    assert len(_capi.SIGNATURES["hop_bin_mf"][1]) == len(_capi.SIGNATURES["hop_bin"][1]) - 1  # no surface
    assert _capi.TIMER_HOP_BIN_MF == 18 and re.search(r"GPLE_TIMER_HOP_BIN_MF\s*=\s*18\b", text)


@pytest.mark.parametrize("name", list(CASES))
def test_at_the_start_a_weight_is_a_count(name):
    """a fresh sample sits on column surface0 of C(x): |c_a|^2 rounds to exactly 2^32 on that surface and to 0 elsewhere"""
    pot, N, start, _ = ensemble(name)
    for grid in grids(start):
        mixed, mf = HD.bin(pot, start, grid), HDM.bin_mf(pot, start, grid)
        counts, coherences, tallies = split(mixed, N, grid)
        weights, mf_coherences, mf_tallies = split(mf, N, grid)
        assert counts.sum() == tallies[0] > 0
        assert np.array_equal(weights, TWO32 * counts) and np.array_equal(mf_coherences, coherences) and np.array_equal(mf_tallies, tallies)


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("bin_all", [False, True])
def test_the_weights_of_a_cell_add_up_to_its_count(name, bin_all):
    """per cell |sum_a weight_a - 2^32 count| <= count (NP / 2 + 1): NP roundings of half a unit, and one unit for the drift of the norm (2^32
    times the 2.6e-14 of DESIGN.md §17 is 1e-4 of it); measured 0, 0 and 8 units for the three ensembles.  The coherence planes and the tallies are the mixed density's, integer for integer"""
    pot, N, _, end = ensemble(name)
    status = end[4]
    assert (status == 0).any() and (name != "dac10" or all((status == s).any() for s in (0, 1, 2)))
    worst = 0
    for grid in grids(end):
        mixed, mf = HD.bin(pot, end, grid, bin_all), HDM.bin_mf(pot, end, grid, bin_all)
        counts, coherences, tallies = split(mixed, N, grid)
        weights, mf_coherences, mf_tallies = split(mf, N, grid)
        count = counts.sum(axis=0)
        assert count.sum() == tallies[0] > 0 and tallies.sum() == (N_TRAJ if bin_all else (status == 0).sum())
        off = np.abs(weights.sum(axis=0) - TWO32 * count)
        worst = max(worst, int(off.max()))
        assert (off <= count * (N / 2.0 + 1.0)).all()
        assert (weights >= 0).all() and (weights.sum(axis=1) > 0).sum() >= 2  # the steps mixed the states: more than one plane holds weight
        assert np.array_equal(mf_coherences, coherences) and coherences.any() and np.array_equal(mf_tallies, tallies)
    print(f"bin_mf {name} bin_all={bin_all}: the sum of a cell's weights is off its count by at most {worst} unit(s) of 2^-32")


def test_the_surface_is_not_read_and_a_status_out_of_range_is_skipped():
    pot, N, _, end = ensemble("dac10")
    grid = grids(end)[2]
    whole = HDM.bin_mf(pot, end, grid, True)
    odd = tuple(a.copy() for a in end)
    odd[3][:] = 7  # no surface is in range: the mixed density would skip everyone
    assert np.array_equal(HDM.bin_mf(pot, odd, grid, True), whole) and HD.bin(pot, odd, grid, True)[-2] == 0
    odd[4][0], odd[4][1] = 3, -1
    skipped = HDM.bin_mf(pot, odd, grid, True)
    assert whole[-2] - skipped[-2] == 2 and skipped[-1] == whole[-1] == 0


def test_a_nan_or_a_huge_value_is_outside():
    pot, N, _, end = ensemble("dac10")
    bad = tuple(a[:4].copy() for a in end)
    bad[4][:] = 0
    for q, values in ((0, [np.nan, 1e300, -1e300, np.inf]), (1, [np.nan, 1e300, -np.inf, 4e18])):
        bad[0][:], bad[1][:] = 0.0, 0.0
        bad[q][:] = values
        acc = HDM.bin_mf(pot, bad, (-6.0, 0.75, 17, -30.0, 1.0, 61))
        assert list(acc[-2:]) == [0, 4] and not acc[:-2].any()


@pytest.mark.parametrize("name", list(CASES))
def test_slices_and_permutations(name):
    pot, N, _, end = ensemble(name)
    grid = grids(end)[1]
    whole = HDM.bin_mf(pot, end, grid, True)
    part = HDM.bin_mf(pot, tuple(a[:100] for a in end), grid, True)
    assert np.array_equal(HDM.bin_mf(pot, tuple(a[100:] for a in end), grid, True, acc=part), whole)
    assert not np.array_equal(part, whole)
    order = np.random.default_rng(3).permutation(N_TRAJ)
    assert np.array_equal(HDM.bin_mf(pot, tuple(a[order] for a in end), grid, True), whole)


@pytest.mark.parametrize("name", list(CASES))
def test_density_is_hermitian_and_normalised(name):
    pot, N, _, end = ensemble(name)
    grid = grids(end)[1]
    acc = HDM.bin_mf(pot, end, grid, True)
    rho = HDM.density_mf(acc, N, grid, N_TRAJ)
    assert rho.shape == (N, N, 16, 9) and acc[N * 16 * 9:-2].any()
    for a in range(N):
        assert not rho[a, a].imag.any() and not np.signbit(rho[a, a].imag).any() and (rho[a, a].real >= 0).all()
        for b in range(N):
            assert np.array_equal(rho[a, b], np.conj(rho[b, a]))  # +0 and -0 compare equal
    upper = split(acc, N, grid)[1]
    pairs = [(a, b) for a in range(N) for b in range(a + 1, N)]
    for q, (a, b) in enumerate(pairs):  # the lower triangle from the negated sum: +0 where the sum is 0
        zero = upper[2 * q + 1].reshape(16, 9) == 0
        assert zero.any() and not np.signbit(rho[b, a].imag[zero]).any() and not np.signbit(rho[a, b].imag[zero]).any()
    total = math.fsum(v for a in range(N) for v in rho[a, a].real.ravel()) * grid[1] * grid[4]  # the sum itself exact
    binned = int(acc[-2])
    assert 0 < binned < N_TRAJ and abs(total - binned / N_TRAJ) <= (N / 2.0 + 1.0) / TWO32 + 4 * EPS
    # the mixed density of the same integers differs on the diagonal alone, by the scale
    mixed = HD.density(acc, N, grid, N_TRAJ)
    for a in range(N):
        for b in range(N):
            if a != b:
                assert np.array_equal(rho[a, b].view(np.uint64), mixed[a, b].view(np.uint64))


@pytest.mark.parametrize("name", list(CASES))
def test_one_cell_against_the_sums(name):
    """the 1 x 1 grid with bin_all holds, times 2^-32, the weights of hop_observe_mf summed over the statuses: n roundings of half a unit, and
    the rounding of two sums of n terms below one"""
    pot, N, _, end = ensemble(name)
    acc = HDM.bin_mf(pot, end, (0.0, 1e3, 1, 0.0, 1e3, 1), True)
    weights = HM.observe(pot, end, MASS)[:3 * N].reshape(3, N).sum(axis=0)
    assert list(acc[-2:]) == [N_TRAJ, 0]
    assert (np.abs(acc[:N] / TWO32 - weights) <= N_TRAJ / (2.0 * TWO32) + 1e-12 * N_TRAJ).all()


# ---- the driver ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["ehrenfest", "fssh"])
def test_driver_with_the_density_from_the_amplitudes(tmp_path, method):
    api = HDM.NumpyHopDensityMfApi()
    res = hopping.run(api, out_dir=str(tmp_path / "out"), phase_grid=(12, 10), phase_density="amplitude", method=method, **RUN)
    n_out = len(res["records"])
    x, p, t = (reconstruct.read_grid(tmp_path / "out" / name) for name in ("x.txt", "p.txt", "t.txt"))
    assert len(x) == 12 and len(p) == 10 and len(t) == n_out > 3 and res["phase_density"] == "amplitude" and res["method"] == method
    blocks = list(reconstruct.phase_blocks(str(tmp_path / "out" / "phase.txt"), 2, 12, 10))
    assert len(blocks) == n_out
    dxdp = (x[1] - x[0]) * (p[1] - p[0])
    mean_field = method == "ehrenfest"
    for rec, block in zip(res["records"], blocks):
        values, lines = reconstruct._parse_host(block)
        assert lines == 4 and len(values) == 2 * 12 * 10 * 4
        rho = values.view(np.complex128).reshape(2, 2, 12, 10)
        running = rec["n_status"][0] if mean_field else rec["counts"][hopping.RUNNING].sum()
        assert rec["binned"] + rec["outside"] == running and rec["outside"] == 0 and "binned_counts" not in rec
        w = rec["binned_weights"]
        assert w.dtype == np.float64 and w.shape == (2,) and abs(w.sum() - rec["binned"]) <= rec["binned"] * 2.0 / TWO32 + 1e-9
        if mean_field:  # the weights of the running trajectories, as hop_observe_mf sums them
            assert np.allclose(w, rec["weights"][0], rtol=0, atol=48 / (2.0 * TWO32) + 1e-10)
        for a in range(2):
            assert np.allclose(rho[a, a].real.sum() * dxdp, w[a] / 48, rtol=1e-4, atol=1e-12) and not rho[a, a].imag.any()
        assert np.allclose(rho[0, 1], np.conj(rho[1, 0]), rtol=1e-5, atol=1e-300)
    assert res["records"][-2]["binned_weights"].min() > 0.01  # both populations from the amplitudes, once the packet has met the crossings
    calls = api.calls
    observe, evolve = ("observe_mf", "evolve_mf") if mean_field else ("observe", "evolve")
    assert calls[0] == ("sample", 48) and calls[1] == ("adiabatic",) and calls[2:5] == [(observe,), ("bin_mf",), ("density_mf",)]
    assert [c[0] for c in calls[2:]] == ([observe, "bin_mf", "density_mf", evolve] * n_out)[:-1]
    # no out_dir: no density is formed
    api2 = HDM.NumpyHopDensityMfApi()
    hopping.run(api2, phase_grid=dict(n_x=1, n_p=1, x_first=0.0, dx=100.0, p_first=0.0, dp=1e4), phase_density="amplitude", method=method, max_outputs=2, **RUN)
    assert [c[0] for c in api2.calls] == ["sample", observe, "bin_mf", evolve, observe, "bin_mf"]


def test_driver_refuses_before_any_call():
    grid = dict(phase_grid=(8, 8))
    for bad in (dict(method="ehrenfest", **grid), dict(method="ehrenfest", phase_density="mixed", **grid),         # the mixed density needs a surface
                dict(method="sqc", phase_density="amplitude", **grid), dict(method="sqc", **grid),                # refused rather than half right
                dict(method="mash", phase_density="amplitude", **grid), dict(method="mash", **grid),
                dict(phase_density="amplitude"), dict(phase_density="mixed"), dict(method="ehrenfest", phase_density="amplitude"),  # no phase_grid
                dict(phase_density="surface", **grid), dict(method="ehrenfest", phase_density="amplitudes", **grid),  # unknown names
                dict(method="ehrenfest", phase_density="amplitude", decoherence="edc", **grid)):
        api = HDM.NumpyHopDensityMfApi()
        with pytest.raises(ValueError):
            hopping.run(api, **{**RUN, **bad})
        assert api.calls == [], bad


def test_the_mixed_density_is_called_as_it_was(tmp_path):
    """method="fssh" with a phase_grid and no phase_density (or "mixed") on the stand-in of tests/hop_density_numpy.py, which has neither
    hop_bin_mf nor hop_density_mf: the calls, the records' keys and the files of the run as it was"""
    assert not hasattr(HD.NumpyHopDensityApi, "hop_bin_mf") and not hasattr(HD.NumpyHopDensityApi, "hop_density_mf")
    runs = {}
    for label, kw in (("none", {}), ("mixed", dict(phase_density="mixed"))):
        api = HD.NumpyHopDensityApi()
        res = hopping.run(api, out_dir=str(tmp_path / label), phase_grid=(12, 10), **kw, **RUN)
        n_out = len(res["records"])
        assert api.calls[0] == ("sample", 48) and api.calls[1] == ("adiabatic",)
        assert [c[0] for c in api.calls[2:]] == (["observe", "bin", "density", "evolve"] * n_out)[:-1]
        assert all("binned_counts" in r and "binned_weights" not in r for r in res["records"])
        runs[label] = (api.calls, res["scattering_line"])
    assert runs["none"] == runs["mixed"]
    for name in ("x.txt", "p.txt", "t.txt", "averages.txt", "phase.txt"):
        assert (tmp_path / "none" / name).read_bytes() == (tmp_path / "mixed" / name).read_bytes()
