"""CPU: the set-up, initial state, output files and final line of the exact MQCLE driver (gaussian_process_liouville_equation_amd/exact_mqcl.py)
against literal values of the reference's liouville_equation/main.cpp, and the properties of the numpy restatement (tests/mqcl_numpy.py) that
DESIGN.md §12 relies on: the roll, the psi form of the hermitised shift, the frequency map and the conserved trace."""
import math

import numpy as np
import pytest

from gaussian_process_liouville_equation_amd import exact_mqcl as EM
from tests import mqcl_numpy as MN

# lnE: (dx, n, dt, TotalStep, OutputTime, OutputStep, Bluestein M), by hand from main.cpp:41-116 and input.py
# lnE = 0: p0 = sqrt(4000) = 63.246, sigma_p = 3.162, p0max = 72.73: 2 pi / 72.73 / 2 = 0.0432 -> 2^-5, n = 30 * 32 + 1 = 961;
#          hbar / 500 / (sigma_p p0 / m) = 1 / 500 / 0.1 = 0.02 -> 2^-6; TotalTime = 30 / 0.031623 * 2 = 1897.37 -> 121431 steps;
#          output time 16 / 0.031623 / 50 = 10.12 -> 20 -> 1280 steps; 2 n - 1 = 1921 -> M = 2048
DEFAULTS = {
    0: (2.0 ** -5, 961, 2.0 ** -6, 121431, 20.0, 1280, 2048),
    1: (2.0 ** -6, 1921, 2.0 ** -8, 294607, 10.0, 2560, 4096),
    2: (2.0 ** -6, 1921, 2.0 ** -9, 357377, 5.0, 2560, 4096),
    3: (2.0 ** -7, 3841, 2.0 ** -10, 433520, 5.0, 5120, 8192),
}


@pytest.mark.parametrize("ln_energy", sorted(DEFAULTS))
def test_setup_defaults(ln_energy):
    dx, n, dt, total, out_time, out_step, M = DEFAULTS[ln_energy]
    s = EM.setup(ln_energy)
    assert (s["dx"], s["n_grids"], s["dt"], s["total_step"], s["output_time"], s["output_step"]) == (dx, n, dt, total, out_time, out_step)
    assert 2 ** math.ceil(math.log2(2 * n - 1)) == M
    assert s["length_x"] == 30.0
    assert s["pmin"] == s["p0"] - math.pi / dx / 2 and s["pmax"] == s["p0"] + math.pi / dx / 2
    assert s["dp"] == (s["pmax"] - s["pmin"]) / (n - 1)
    assert s["sigma_x"] == 1.0 / 2.0 / s["sigma_p"]


def literal_grid(lo, hi, n):
    """main.cpp:89, 91 one point at a time, in Python floats"""
    return np.array([(lo * (n - 1 - i) + hi * i) / (n - 1) for i in range(n)])


def test_grids_follow_the_interpolation_formula():
    s = EM.setup(0.0)
    n = s["n_grids"]
    x, p = literal_grid(s["xmin"], s["xmax"], n), literal_grid(s["pmin"], s["pmax"], n)
    assert np.array_equal(s["x"], x) and np.array_equal(s["p"], p)
    # p is not pmin + dp j at 546 of 961 points; x is xmin + dx i everywhere (dyadic dx, integer bounds) ...
    assert int(np.sum(p != s["pmin"] + s["dp"] * np.arange(n))) == 546
    assert np.array_equal(x, s["xmin"] + s["dx"] * np.arange(n))
    # ... but not on a box with fractional bounds
    b = EM.setup(0.0, xmin=-10.3, xmax=9.1, dx=(9.1 - -10.3) / 960)
    assert b["n_grids"] == 961
    xb = literal_grid(-10.3, 9.1, 961)
    assert np.array_equal(b["x"], xb)
    assert int(np.sum(xb != -10.3 + b["dx"] * np.arange(961))) == 755


def test_initial_density_is_normalised():
    s = EM.setup(0.0)
    rho = EM.initial_density(s["x"], s["p"], s["dx"], s["dp"], s["x0"], s["p0"], s["sigma_x"], s["sigma_p"], 2)
    assert abs(rho[0, 0].real.sum() * s["dx"] * s["dp"] - 1.0) <= 1e-14
    assert not rho[0, 1].any() and not rho[1, 0].any() and not rho[1, 1].any() and not rho.imag.any()


def small_grid(n, lx=20.0):
    i = np.arange(n, dtype=np.float64)
    return (-10.0 * (n - 1 - i) + 10.0 * i) / (n - 1), (5.0 * (n - 1 - i) + 45.0 * i) / (n - 1), lx


@pytest.mark.parametrize("n", [9, 10, 33])
def test_shift_by_whole_points_is_a_roll(n):
    x, p, lx = small_grid(n)
    rho = MN.random_hermitian(2, n, np.random.default_rng(n))
    mass, m = 2000.0, 3
    # one common distance for every column: p_j / mass * t = m L / n
    pcol = np.full(n, 25.0)
    t = m * lx / n * mass / 25.0
    out = MN.position(rho, pcol, mass, lx, t)
    assert np.abs(out - np.roll(rho, m, axis=2)).max() <= 1e-13 * np.abs(rho).max()


@pytest.mark.parametrize("n", [9, 10, 961])
def test_hermitised_shift_is_the_psi_multiplier(n):
    rng = np.random.default_rng(5)
    num_pes = 2
    rho = MN.random_hermitian(num_pes, n, rng)
    p = rng.uniform(10, 40, n)
    mass, lx, t = 2000.0, 20.0, 37.0
    lit = MN.position(rho, p, mass, lx, t)
    f = MN.ref_freq(n)
    theta = lambda ff: -p[None, :] / mass * 2 * ff[:, None] * MN.PI / lx * t
    phi = np.exp(1j * theta(f))                                      # (k, j)
    psi = 0.5 * (phi + np.conj(phi[(-np.arange(n)) % n]))
    assert np.abs(psi - MN.psi_multiplier(lambda ff: theta(ff), n)).max() <= 1e-15
    for a in range(num_pes):
        for b in range(a, num_pes):
            v = np.fft.ifft(psi * np.fft.fft(rho[a, b], axis=0), axis=0)
            if a == b:
                v = v.real + 0j
            assert np.abs(v - lit[a, b]).max() <= 1e-14 * np.abs(rho).max()
    if n % 2:
        assert np.abs(np.abs(psi) - 1).max() > 1e-3  # not unitary at the top frequencies for odd n


def test_frequency_map():
    for n in (9, 127, 961):
        assert not np.array_equal(MN.ref_freq(n), MN.fftfreq(n))
        assert MN.ref_freq(n)[(n - 1) // 2] == -(n + 1) // 2
    for n in (10, 64, 100):
        assert np.array_equal(MN.ref_freq(n), MN.fftfreq(n))


def test_restatement_conserves_trace():
    n = 33
    x, p, lx = small_grid(n)
    rho = MN.random_hermitian(3, n, np.random.default_rng(1))
    bases = MN.Bases(x, 3, 3)
    out = MN.evolve(rho, bases, p, 2000.0, lx, 40.0, 0.5, 5)
    tr = lambda r: sum(r[a, a].real.sum() for a in range(3))
    assert abs(tr(out) - tr(rho)) <= 1e-12 * np.abs(rho).sum()


def row_sums(r):
    """sum over p of sum_a Re rho_aa, per x row"""
    return sum(r[a, a].real.sum(axis=1) for a in range(r.shape[0]))


def column_sums(r):
    """sum over x of sum_a Re rho_aa, per p column"""
    return sum(r[a, a].real.sum(axis=0) for a in range(r.shape[0]))


@pytest.mark.parametrize("axis", ["rows", "columns"])
@pytest.mark.parametrize("num_pes, model, n", [(2, 1, 37), (3, 3, 40)])
def test_decoupled_limits_evolve_rows_and_columns_on_their_own(num_pes, model, n, axis):
    """what tests/test_gpu_mqcl_sizes.py rests on at n up to 4096: with mass = DECOUPLE (length_p = DECOUPLE) R (P) is the identity, a subset of
    rows (columns) restated alone is the full restatement on that subset, and the sums along the propagated axis are conserved one by one"""
    x, p, lx = small_grid(n)
    lp, mass, dt, steps = 40.0, 2000.0, 2.0, 2
    rho = MN.random_hermitian(num_pes, n, np.random.default_rng(100 * num_pes + n))
    bases = MN.Bases(x, model, num_pes)
    idx = np.array([0, 1, 5, 17, n - 2, n - 1])
    scale = np.abs(rho).max()
    if axis == "rows":
        full = MN.evolve(rho, bases, p, MN.DECOUPLE, lx, lp, dt, steps)
        subset = lambda freq: MN.evolve_rows(rho[:, :, idx, :], x[idx], p, model, num_pes, lx, lp, dt, steps, freq=freq)
        picked, sums = full[:, :, idx, :], row_sums
    else:
        full = MN.evolve(rho, bases, p, mass, lx, MN.DECOUPLE, dt, steps)
        subset = lambda freq: MN.evolve_columns(rho[:, :, :, idx], bases, p[idx], mass, lx, dt, steps, freq=freq)
        picked, sums = full[:, :, :, idx], column_sums
    sub = subset(MN.ref_freq)
    assert np.abs(sub - picked).max() <= 1e-14 * scale, np.abs(sub - picked).max() / scale
    s0, s1 = sums(rho), sums(full)
    assert np.abs(s1 - s0).max() <= 1e-13 * np.abs(s0).max(), np.abs(s1 - s0).max() / np.abs(s0).max()
    # not a test of the identity: the surviving propagators move the state
    assert np.abs(full - rho).max() > 1e-2 * scale
    if n % 2:
        other = subset(MN.fftfreq)
        assert np.abs(other - sub).max() > 1e-9 * scale, np.abs(other - sub).max() / scale


class NumpyApi:
    """the three gple_mqcl_* calls and pes_adiabatic_n on the restatement: the driver's loop and files without a GPU"""

    def pes_adiabatic_n(self, num_pes, model, x):
        return MN.ON.adiabatic(x, model, num_pes)[0], None, None

    def mqcl_transform(self, num_pes, model, x, rho, frm, to):
        return MN.transform(rho, MN.Bases(x, model, num_pes), frm, to)

    def mqcl_evolve(self, num_pes, model, x, p, rho, mass, length_x, length_p, dt, n_steps):
        return MN.evolve(rho, MN.Bases(x, model, num_pes), p, mass, length_x, length_p, dt, n_steps)

    def mqcl_observe(self, num_pes, model, x, p, rho, mass, dx, dp):
        return MN.observe(rho, MN.Bases(x, model, num_pes), x, p, mass, dx, dp)


KW = dict(dx=0.5, dt=1.0, xmin=-10.0, xmax=10.0, x0=-0.5, output_time=20.0)


def test_driver_files_and_final_line_when_the_loop_runs_out(tmp_path):
    res = EM.run(NumpyApi(), model=1, num_pes=2, out_dir=str(tmp_path), max_outputs=1, **KW)
    s = res["setup"]
    assert s["n_grids"] == 41 and not res["stopped"] and res["final_basis"] == EM.DIABATIC
    assert open(tmp_path / "x.txt").read() == "".join("%g\n" % v for v in s["x"])
    assert open(tmp_path / "p.txt").read() == "".join("%g\n" % v for v in s["p"])
    assert open(tmp_path / "t.txt").read() == "0\n20\n"
    lines = open(tmp_path / "averages.txt").read().splitlines()
    assert len(lines) == 2 and len(lines[1].split()) == 6
    r = res["records"][1]
    assert lines[1] == " ".join("%g" % v for v in [r["t"], r["E"], r["x"], r["p"], *r["populations"]])
    phase = open(tmp_path / "phase.txt").read()
    blocks = phase.split("\n\n")
    assert blocks[-1] == "" and len(blocks) == 3
    first = blocks[0].split("\n")
    assert len(first) == 4 and all(len(line.split()) == 2 * 41 * 41 for line in first)
    # the loop ran out: the final line carries the populations of the DIABATIC state
    dia = EM.populations(res["rho"], s["dx"], s["dp"])
    assert res["final_line"] == " ".join("%g" % v for v in [math.log(s["p0"] ** 2 / 2 / s["mass"]), *dia])
    assert not np.allclose(dia, r["populations"], atol=1e-6)


def test_driver_final_line_when_the_stop_criterion_fires(tmp_path):
    res = EM.run(NumpyApi(), model=2, num_pes=2, out_dir=str(tmp_path), write_phase=None, **KW)
    assert res["stopped"] and res["final_basis"] == EM.ADIABATIC
    last = res["records"][-1]
    assert last["x"] > 0.5 and len(res["records"]) == 3
    s = res["setup"]
    assert res["final_line"] == " ".join("%g" % v for v in [s["p0"], *last["populations"]])  # ECR: p0, adiabatic populations
    assert not (tmp_path / "phase.txt").exists()


def test_stop_criterion():
    assert EM.stop_criterion(0.6, 0.4, 63.0, -0.5)          # beyond -x0
    assert EM.stop_criterion(0.3, 0.4, 63.0, -8.0)          # turned back
    assert not EM.stop_criterion(0.3, 0.2, 63.0, -8.0)
    assert not EM.stop_criterion(-0.1, 0.2, 63.0, -8.0)     # x <= 0
