"""CPU: the set-up of the exact DVR driver (gaussian_process_liouville_equation_amd/exact.py) at the defaults of the reference's
schrodinger_equation/input.py, its file writers, and the numpy restatement of the Wigner sum (tests/dvr_numpy.py) against the analytic
Wigner function of a Gaussian."""
import math
import os

import numpy as np
import pytest

from tests import dvr_numpy as DN


@pytest.mark.parametrize("ln_e, dx, n_grids", [
    # p0 = sqrt(2 m e^lnE), p0max = p0 + 3 p0 / 20; dx = 2^floor(log2(min(0.1, 2 pi / p0max / 5)))  (main.cpp:74); n = 30 / dx + 1
    (-4.0, 2.0 ** -4, 481),   # p0 = 8.5594: 2 pi / 9.843 / 5 = 0.1277 -> min with 0.1 -> 1/16
    (0.0, 2.0 ** -6, 1921),   # p0 = 63.246: 0.01728 -> 1/64
    (1.0, 2.0 ** -7, 3841),   # p0 = 104.27: 0.01048 -> 1/128
])
def test_setup_at_input_py_defaults(ln_e, dx, n_grids):
    from gaussian_process_liouville_equation_amd import exact

    s = exact.setup(ln_e)
    p0 = math.sqrt(2.0 * 2000.0 * math.exp(ln_e))
    assert s["p0"] == pytest.approx(p0, rel=1e-15)
    assert s["sigma_x"] == pytest.approx(1.0 / (2.0 * p0 / 20.0), rel=1e-15)
    assert s["dx"] == dx
    assert s["n_grids"] == n_grids
    assert s["x"][0] == -15.0 and s["x"][-1] == pytest.approx(15.0, abs=1e-12)
    # p range: p0 -+ pi hbar / dx / 2 (main.cpp:103-104), n_grids points
    assert len(s["p"]) == n_grids
    assert s["p"][0] == pytest.approx(p0 - math.pi / dx / 2, rel=1e-14)
    assert s["p"][-1] == pytest.approx(p0 + math.pi / dx / 2, rel=1e-14)
    # input.py: total time (-x0 - x0) / (p0 / m) = 16 m / p0, divided by 50 outputs, rounded by its 1-2-5 rule (int() truncates)
    raw = 16.0 * 2000.0 / p0 / 50.0
    lg = math.log10(raw)
    resume = lg - int(lg)
    expect = (2 if resume < 0.3 else 5 if resume < 0.7 else 10) * 10.0 ** int(lg)
    assert s["output_time"] == pytest.approx(expect) and s["dt"] == s["output_time"]
    # main.cpp:127, 144-145: total time = 30 / (p0 / m) * 2, steps = floor(total / dt), one step per output
    assert s["total_step"] == int(60.0 * 2000.0 / p0 / s["dt"])
    assert s["output_step"] == 1


def test_setup_hand_values():
    """The three default grids worked out by hand: ln E = -4, 0, 1 give dt = 100, 20, 10 and 140, 94, 115 steps."""
    from gaussian_process_liouville_equation_amd import exact

    # ln E = -4: p0 = 8.5594, 16 * 2000 / p0 / 50 = 74.77 -> lg 1.874, resume 0.874 -> 10 * 10 = 100; 120000 / 8.5594 / 100 = 140.2 -> 140
    # ln E = 0:  p0 = 63.2456, 10.119 -> lg 1.005, resume 0.005 -> 2 * 10 = 20; 120000 / 63.2456 / 20 = 94.87 -> 94
    # ln E = 1:  p0 = 104.275, 6.138 -> lg 0.788 -> 10 * 1 = 10; 120000 / 104.275 / 10 = 115.08 -> 115
    for ln_e, dt, steps in ((-4.0, 100.0, 140), (0.0, 20.0, 94), (1.0, 10.0, 115)):
        s = exact.setup(ln_e)
        assert s["dt"] == pytest.approx(dt) and s["total_step"] == steps, (ln_e, s["dt"], s["total_step"])


def test_restated_wigner_of_a_grid_gaussian_is_analytic():
    """Guards the helper itself: the discrete Wigner sum of a normalised grid Gaussian on the default ln E = -4 grid (n = 481) equals
    W = exp(-(x - x0)^2 / (2 sx^2) - 2 sx^2 (p - p0)^2 / hbar^2) / (pi hbar) for both boundaries."""
    from gaussian_process_liouville_equation_amd import exact

    s = exact.setup(-4.0)
    # centred in the box: the sum stops at the walls (reflective) or takes the other end of the box there (periodic), which cuts the integrand
    # exp(-((x - x0)^2 + y^2) / (2 sx^2)) at |y| = min(x - xmin, xmax - x); at x0 = 0 that is >= 12.8 sx for the rows that carry weight (at the
    # reference's x0 = -8 it is 6 sx, a cut of e^-18 relative)
    x0 = 0.0
    psi = DN.gaussian(s["x"], x0, s["p0"], s["sigma_x"])
    W = DN.analytic_wigner(s["x"], s["p"], x0, s["p0"], s["sigma_x"])
    P, _ = DN.wigner(psi, 1, DN.REFLECTIVE, s["dx"], s["p"], dtype=np.complex128)
    assert np.abs(P[0, 0] - W).max() <= 1e-10 * W.max()
    # periodic: rows whose k-range wraps round the box pair x - y on one side with x + y on the other, and near the walls that pair meets the
    # packet from both ends (the second packet general.cpp:373 warns of); on the rows whose k-range stays inside the box the sums agree
    P, _ = DN.wigner(psi, 1, DN.PERIODIC, s["dx"], s["p"], dtype=np.complex128)
    K, n = DN.half_range(DN.PERIODIC, s["n_grids"]), s["n_grids"]
    inside = slice(K, n - K)
    assert W[inside].max() == W.max()
    assert np.abs(P[0, 0] - W)[inside].max() <= 1e-10 * W.max()


def test_writers_follow_the_reference_layout(tmp_path):
    from gaussian_process_liouville_equation_amd import exact

    num_pes, n, n_p, T = 2, 5, 3, 2
    rng = np.random.default_rng(1)
    P = rng.normal(size=(T, num_pes, num_pes, n, n_p)) + 1j * rng.normal(size=(T, num_pes, num_pes, n, n_p))
    exact.write_grid(tmp_path / "x.txt", np.linspace(-1, 1, n))
    lines = open(tmp_path / "x.txt").read().splitlines()
    assert len(lines) == n and all(len(l.split()) == 1 for l in lines)
    text = "".join(exact.phase_block(P[t]) for t in range(T))
    lines = text.split("\n")
    # per output time: num_pes^2 element lines of 2 n n_p numbers, then one blank line
    per = num_pes * num_pes + 1
    assert len(lines) == T * per + 1 and lines[-1] == ""
    for t in range(T):
        block = lines[t * per:(t + 1) * per]
        assert block[-1] == ""
        for e, line in enumerate(block[:-1]):
            assert line.startswith(" ")
            vals = np.array([float(v) for v in line.split()])
            assert len(vals) == 2 * n * n_p
            i, j = divmod(e, num_pes)
            ref = P[t, i, j].reshape(-1)
            assert np.allclose(vals[0::2], ref.real, rtol=1e-5) and np.allclose(vals[1::2], ref.imag, rtol=1e-5)
    psi = rng.normal(size=num_pes * n) + 1j * rng.normal(size=num_pes * n)
    line = exact.psi_line(psi)
    assert line.endswith("\n") and len(line.split()) == num_pes * n
    assert np.allclose([float(v) for v in line.split()], np.abs(psi) ** 2, rtol=1e-5)
    line = exact.averages_line(10.0, 1.0, 2.0, 3.0, [0.5, 0.5], [4.0, 5.0, 6.0])
    assert line.split() == ["10", "1", "2", "3", "0.5", "0.5", "4", "5", "6"]


def test_diabatic_adiabatic_round_trip():
    from gaussian_process_liouville_equation_amd import exact
    from oracle import evolve_oracle_n as ON

    x = np.linspace(-5, 5, 7)
    _, C, _, _ = ON.adiabatic(x, 1, 2)
    psi = exact.initial_adiabatic_psi(x, -1.0, 3.0, 1.0, 2)
    assert np.allclose(exact.to_adiabatic(exact.to_diabatic(psi, C), C), psi, atol=1e-15)
    assert not os.path.exists("phase.txt")
