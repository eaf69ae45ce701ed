"""CPU: the numpy restatement of gple_hop_bin / gple_hop_density (tests/hop_density_numpy.py), which the GPU tests lean on, the driver
hopping.run(phase_grid=...) on a numpy stand-in api, and the new symbols of the built library (the test here that fails without the feature)."""
import functools
import math
import os
import re

import numpy as np
import pytest

import gaussian_process_liouville_equation_amd as pkg
from gaussian_process_liouville_equation_amd import _capi, hopping, reconstruct
from tests import hop_density_numpy as HD
from tests import hop_numpy as HN
from tests.conftest import ROOT

EPS = np.finfo(np.float64).eps
MASS, SEED = 2000.0, 20250117


@functools.lru_cache(maxsize=None)
def ensemble(name):
    """(potential, N, state): 293 trajectories as tests/test_gpu_hop.py evolves them; "dac10" has finished ones on either side"""
    model, N, p0, dt, steps, surface0 = {"dac10": (HN.DAC, 2, 10.0, 2.0, 900, 0), "tsac": (HN.TSAC, 3, 10.0, 4.0, 250, 1)}[name]
    pot = HN.builtin(model, N)
    start = HN.sample(pot, N, 293, SEED, -4.0, p0, 1.0 / (2.0 * p0 / 20.0), p0 / 20.0, surface0=surface0)
    end, _ = HN.evolve(pot, start, SEED, MASS, dt, 0, steps, -6.0, 6.0)
    return pot, N, end


def grid_over(state, n_x, n_p, margin=0.0):
    """a grid of n_x x n_p points whose cells cover [-6, 6] and the ensemble's momenta, less `margin` of the momentum range at either end"""
    p = state[1]
    lo, hi = p.min() + margin * (p.max() - p.min()), p.max() - margin * (p.max() - p.min())
    dx, dp = 12.0 / max(1, n_x - 1), max(hi - lo, 1.0) / max(1, n_p - 1)
    return (-6.0 if n_x > 1 else 0.0, dx if n_x > 1 else 1e3, n_x, lo if n_p > 1 else 0.0, dp if n_p > 1 else 1e3, n_p)


def test_the_library_exports_and_the_binding_declares_the_density_entry_points():
    lib = pkg.load_library()  # no HIP call at load time: works without a GPU
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gple.h")).read(), flags=re.S)
    for name in ("hop_bin", "hop_density"):
        assert re.search(r"\bint\s+gple_%s\s*\(" % name, text), name
        assert name in _capi.GPLE_SYMBOLS
        f = getattr(lib, "gple_" + name)
        assert f.argtypes is not None and len(f.argtypes) == len(_capi.SIGNATURES[name][1])
    assert all(hasattr(_capi.Api, m) for m in ("hop_bin", "hop_density"))
    assert (_capi.HOP_ACCUMULATE, _capi.HOP_BIN_ALL, _capi.TIMER_HOP_BIN) == (0x4000, 0x8000, 13)
    assert re.search(r"GPLE_TIMER_HOP_BIN\s*=\s*13\b", text) and re.search(r"GPLE_HOP_ACCUMULATE\s+0x4000u", text) and re.search(r"GPLE_HOP_BIN_ALL\s+0x8000u", text)


@pytest.mark.parametrize("name", ["dac10", "tsac"])
@pytest.mark.parametrize("bin_all", [False, True])
def test_tallies(name, bin_all):
    pot, N, state = ensemble(name)
    status = state[4]
    selected = len(status) if bin_all else int((status == 0).sum())
    for grid in (grid_over(state, 16, 9), grid_over(state, 1, 1), grid_over(state, 16, 9, margin=0.2)):
        acc = HD.bin(pot, state, grid, bin_all)
        n_cells = grid[2] * grid[5]
        binned, outside = acc[-2:]
        assert binned + outside == selected and acc[:N * n_cells].sum() == binned and (acc[:N * n_cells] >= 0).all()
    assert outside > 0 and binned > 0  # the last grid leaves some outside
    # a trajectory whose surface or status is out of range is skipped: neither binned nor outside
    odd = tuple(a.copy() for a in state)
    odd[3][0], odd[4][1] = N, 3
    whole, skipped = HD.bin(pot, state, grid_over(state, 1, 1), True), HD.bin(pot, odd, grid_over(state, 1, 1), True)
    assert whole[-2] - skipped[-2] == 2 and skipped[-1] == whole[-1] == 0


def test_a_nan_or_a_huge_value_is_outside():
    pot, N, state = ensemble("dac10")
    bad = tuple(a[:4].copy() for a in state)
    bad[4][:] = 0
    bad[0][:] = [np.nan, 1e300, -1e300, np.inf]
    acc = HD.bin(pot, bad, (-6.0, 0.75, 17, -30.0, 1.0, 61))
    assert list(acc[-2:]) == [0, 4] and not acc[:-2].any()
    bad[0][:] = 0.0
    bad[1][:] = [np.nan, 1e300, -np.inf, 4e18]
    acc = HD.bin(pot, bad, (-6.0, 0.75, 17, -30.0, 1.0, 61))
    assert list(acc[-2:]) == [0, 4] and not acc[:-2].any()


@pytest.mark.parametrize("name", ["dac10", "tsac"])
def test_density_is_hermitian_and_normalised(name):
    pot, N, state = ensemble(name)
    grid = grid_over(state, 16, 9, margin=0.1)
    acc = HD.bin(pot, state, grid, True)
    assert acc[N * grid[2] * grid[5]:-2].any()  # coherences are there
    n_norm = len(state[0])
    rho = HD.density(acc, N, grid, n_norm)
    assert rho.shape == (N, N, 16, 9)
    for a in range(N):
        assert not rho[a, a].imag.any() and not np.signbit(rho[a, a].imag).any()
        for b in range(N):
            assert np.array_equal(rho[a, b], np.conj(rho[b, a]))  # +0 and -0 compare equal
    total = math.fsum(v for a in range(N) for v in rho[a, a].real.ravel()) * grid[1] * grid[4]  # the sum itself exact
    assert 0 < acc[-2] < n_norm and abs(total - acc[-2] / n_norm) <= 4 * EPS * acc[-2] / n_norm


@pytest.mark.parametrize("name", ["dac10", "tsac"])
def test_slices_and_permutations(name):
    pot, N, state = ensemble(name)
    grid = grid_over(state, 16, 9, margin=0.1)
    whole = HD.bin(pot, state, grid, True)
    part = HD.bin(pot, tuple(a[:100] for a in state), grid, True)
    assert np.array_equal(HD.bin(pot, tuple(a[100:] for a in state), grid, True, acc=part), whole)
    assert not np.array_equal(part, whole)
    order = np.random.default_rng(3).permutation(len(state[0]))
    assert np.array_equal(HD.bin(pot, tuple(a[order] for a in state), grid, True), whole)


def test_the_sample_against_its_law():
    """65536 draws of the packet into 7 x 5 cells of a sigma_x by 1.5 sigma_p: every count lies within 6 sqrt(n q (1 - q)) + 1 of n q, q the cell's
    probability from erf (six binomial standard deviations, and one for the rounding of an edge).  Measured: the worst cell at 0.36 of the
    bound, 39 points outside.  At the start c = C^T b is a unit vector of the adiabatic basis to rounding: every coherence term rounds to 0"""
    n, x0, p0 = 65536, -4.0, 16.0
    sp = p0 / 20.0
    sx = 1.0 / (2.0 * sp)
    pot = HN.builtin(HN.DAC, 2)
    state = HN.sample(pot, 2, n, 0, x0, p0, sx, sp)
    dx, dp = sx, 1.5 * sp
    grid = (x0 - 3 * dx, dx, 7, p0 - 2 * dp, dp, 5)
    acc = HD.bin(pot, state, grid)
    Phi = lambda z: 0.5 * (1.0 + math.erf(z / math.sqrt(2.0)))
    qx = [Phi((grid[0] + (i + 0.5) * dx - x0) / sx) - Phi((grid[0] + (i - 0.5) * dx - x0) / sx) for i in range(7)]
    qp = [Phi((grid[3] + (j + 0.5) * dp - p0) / sp) - Phi((grid[3] + (j - 0.5) * dp - p0) / sp) for j in range(5)]
    q = np.outer(qx, qp)
    counts = acc[:35].reshape(7, 5)
    ratio = np.abs(counts - n * q) / (6.0 * np.sqrt(n * q * (1.0 - q)) + 1.0)
    print(f"sample against its law: worst cell at {ratio.max():.3g} of the bound, {acc[-1]} outside")
    assert (ratio <= 1.0).all()
    assert not acc[35:70].any() and not acc[70:-2].any()  # nobody on the upper surface, and no coherence
    assert acc[-2] + acc[-1] == n and abs(acc[-1] - n * (1.0 - q.sum())) <= 6.0 * math.sqrt(n * (1.0 - q.sum())) + 1.0


def test_driver_writes_what_reconstruct_reads(tmp_path):
    api = HD.NumpyHopDensityApi()
    kw = dict(model=hopping.DAC, num_pes=2, ln_energy=-2.0, n_traj=48, seed=4, dt=4.0, x0=-4.0, xmin=-6.0, xmax=6.0)
    res = hopping.run(api, out_dir=str(tmp_path / "with"), phase_grid=(12, 10), **kw)
    s, n_out = res["setup"], len(res["records"])
    x, p, t = (reconstruct.read_grid(tmp_path / "with" / name) for name in ("x.txt", "p.txt", "t.txt"))
    assert len(x) == 12 and len(p) == 10 and len(t) == n_out > 3
    assert np.allclose(x, np.linspace(-6.0, 6.0, 12), rtol=1e-5) and np.allclose(p, -p[::-1], rtol=1e-5)
    E = HN.states(np.linspace(-6.0, 6.0, 12), HN.builtin(HN.DAC, 2))[1]
    p_max = math.sqrt((s["p0"] + 6.0 * s["sigma_p"]) ** 2 + 2.0 * s["mass"] * (E.max() - E.min()))
    assert abs(p[-1] - p_max) <= 1e-5 * p_max
    blocks = list(reconstruct.phase_blocks(str(tmp_path / "with" / "phase.txt"), 2, 12, 10))
    assert len(blocks) == n_out
    dxdp = (x[1] - x[0]) * (p[1] - p[0])
    for rec, block in zip(res["records"], blocks):
        values, lines = reconstruct._parse_host(block)
        assert lines == 4 and len(values) == 2 * 12 * 10 * 4
        rho = values.view(np.complex128).reshape(2, 2, 12, 10)
        running = rec["counts"][hopping.RUNNING]
        assert rec["binned"] + rec["outside"] == running.sum() and rec["outside"] == 0  # the momentum axis is a bound
        assert np.array_equal(rec["binned_counts"], running)
        assert np.allclose(rho[0, 0].real.sum() * dxdp, running[0] / 48, rtol=1e-4, atol=1e-12)
        assert np.allclose(rho[0, 1], np.conj(rho[1, 0]), rtol=1e-5, atol=1e-300)
    # per output one bin and one density behind the observe; the energies once, before anything else that follows the sample
    calls = api.calls
    assert calls[0] == ("sample", 48) and calls[1] == ("adiabatic",) and calls[2:5] == [("observe",), ("bin",), ("density",)]
    assert sum(c == ("bin",) for c in calls) == sum(c == ("density",) for c in calls) == n_out
    # without a grid: the calls and the files of the run as it was
    plain_api = HN.NumpyHopApi()
    plain = hopping.run(plain_api, out_dir=str(tmp_path / "without"), **kw)
    assert sorted(os.listdir(tmp_path / "without")) == ["averages.txt", "t.txt"]
    assert plain_api.calls == [c for c in calls if c[0] in ("sample", "observe", "evolve")]
    assert all("binned" not in r for r in plain["records"]) and plain["scattering_line"] == res["scattering_line"]
    for name in ("t.txt", "averages.txt"):
        assert open(tmp_path / "without" / name).read() == open(tmp_path / "with" / name).read()
    # a dict overrides; no out_dir: no density is formed
    api2 = HD.NumpyHopDensityApi()
    res2 = hopping.run(api2, phase_grid=dict(n_x=1, n_p=1, x_first=0.0, dx=100.0, p_first=0.0, dp=1e4), max_outputs=2, **kw)
    assert [c[0] for c in api2.calls] == ["sample", "observe", "bin", "evolve", "observe", "bin"]
    assert all(r["binned"] == r["counts"][hopping.RUNNING].sum() for r in res2["records"])
    for bad in ((4,), dict(n_x=4), dict(n_x=4, n_p=4, nx=3), dict(n_x=1, n_p=4)):
        with pytest.raises(ValueError):
            hopping.run(HD.NumpyHopDensityApi(), phase_grid=bad, max_outputs=1, **kw)
