"""CPU: the host pieces of the reconstruction driver (gaussian_process_liouville_equation_amd/reconstruct.py) against
hand-computed values, the numpy restatement tests/recon_numpy.py against small cases worked by hand, and the register budget of the
contraction kernel from the cross-compiled ISA."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from gaussian_process_liouville_equation_amd import reconstruct as R
from tests import mqcl_numpy as MN
from tests import recon_numpy as RN
from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "gaussian_process_liouville_equation_amd", "csrc")


def survey_rows(rows):
    s = np.zeros((len(rows), 8))
    for q, (mx, mn, arg) in enumerate(rows):
        s[q, 0], s[q, 1], s[q, 3] = mx, mn, arg
    return s


def test_set_initial_value_and_is_small():
    x, p = np.linspace(-10.0, 10.0, 5), np.linspace(10.0, 30.0, 4)
    s = survey_rows([(0.5, 0.0, 2 * 4 + 1), (0.02, -0.004, 3), (0.009, -0.009, 0), (0.009, -0.02, -1)])
    assert R.is_small(s).tolist() == [False, False, True, False]  # max < 1e-2 and min > -1e-2 (gpr.cpp:206)
    lower, upper, start = R.set_initial_value(s, x, p, 2)
    sigma_p = p[1] / 20.0  # the maximum of plane 0 sits at (ix, ip) = (2, 1)
    assert lower.shape == upper.shape == start.shape == (4, 4)
    for q in range(4):
        assert lower[q].tolist() == [1e-8, 1e-4, 1.0 / 20.0, 1.0 / 20.0]
        assert upper[q, :2].tolist() == [1e-5, 1.0] and np.all(upper[q, 2:] == np.finfo(np.float64).max)
        assert start[q].tolist() == [1e-8, 1.0, 1.0 / (0.5 / sigma_p), 1.0 / sigma_p]
    with pytest.raises(ValueError):
        R.set_initial_value(survey_rows([(0.0, -1.0, -1)] * 4), x, p, 2)


def test_population_and_kinetic_energy_from_gpr():
    hyper = np.array([1e-6, 0.5, 2.0, 0.25])  # w_g = 0.5, a_x = 2, a_p = 1 / 4
    X = np.array([[0.0, 3.0], [1.0, -1.0], [2.0, 2.0]])
    b = np.array([1.0, -2.0, 4.0])
    coe = 2.0 * math.pi * 0.25 / 0.5
    assert R.population_from_gpr(hyper, b) == pytest.approx(coe * 3.0, rel=1e-15)
    # row vector P_i^2 + a_p^-2 = (25, 17, 20)
    assert R.kinetic_energy_from_gpr(hyper, X, b, 2000.0) == pytest.approx(coe * (25.0 - 34.0 + 80.0) / 4000.0, rel=1e-15)


def test_obey_conservation():
    # one surface: the normalisation alone
    f, singular = R.obey_conservation(np.array([0.8, 0.0]), np.array([0.03, 0.0]), np.array([False, True]), 0.05)
    assert f.tolist() == [1.25, 1.0] and not singular
    # two surfaces: [0.6 0.3; 0.03 0.027] c = [1; 0.05] by Cramer's rule
    pop, en = np.array([0.6, 0.3]), np.array([0.03, 0.027])
    f, singular = R.obey_conservation(pop, en, np.array([False, False]), 0.05)
    det = 0.6 * 0.027 - 0.3 * 0.03
    c0, c1 = (0.027 - 0.3 * 0.05) / det, (0.6 * 0.05 - 0.03) / det
    assert not singular and f[0] == pytest.approx(c0, rel=1e-13) and f[1] == pytest.approx(c1, rel=1e-13)
    assert f @ pop == pytest.approx(1.0, rel=1e-13) and f @ en == pytest.approx(0.05, rel=1e-13)
    # three surfaces split 1 + 2 (gpr.cpp:970: i < 3 / 2 goes to the first factor): levels 1 and 2 share theirs
    pop, en = np.array([0.5, 0.2, 0.1]), np.array([0.02, 0.03, 0.01])
    f, singular = R.obey_conservation(pop, en, np.array([False, False, False]), 0.07)
    det = 0.5 * 0.04 - 0.3 * 0.02
    c0, c1 = (0.04 - 0.3 * 0.07) / det, (0.5 * 0.07 - 0.02) / det
    assert not singular and f[1] == f[2] and f[0] == pytest.approx(c0, rel=1e-13) and f[1] == pytest.approx(c1, rel=1e-13)
    # three levels, the middle one 0 everywhere: levels 0 and 2 make the two halves, level 1 keeps 1
    f, singular = R.obey_conservation(pop, en, np.array([False, True, False]), 0.07)
    assert not singular and f[1] == 1.0 and f[0] * 0.5 + f[2] * 0.1 == pytest.approx(1.0, rel=1e-13)
    # singular: energy proportional to population
    f, singular = R.obey_conservation(np.array([0.6, 0.3]), np.array([0.06, 0.03]), np.array([False, False]), 0.05)
    assert singular and f.tolist() == [1.0, 1.0]
    f, singular = R.obey_conservation(np.array([0.0, 0.0]), np.array([0.0, 0.0]), np.array([True, True]), 0.05)
    assert not singular and f.tolist() == [1.0, 1.0]


class EnergyStub:
    """pes_adiabatic_n of the library from the oracle's potentials (no GPU here)"""

    def pes_adiabatic_n(self, num_pes, model, x):
        return (MN.Bases(np.asarray(x), model, num_pes).E,)


@pytest.mark.parametrize("hyper", [[1e-6, 0.8, 1.0 / 0.7, 0.25], [1e-6, 0.3, 2.5, 1.0], [1e-6, 1.0, 0.4, 0.05]])
def test_potential_energy_from_gpr_against_quad(hyper):
    from scipy.integrate import quad
    hyper = np.array(hyper)
    rng = np.random.default_rng(31)
    X = np.stack([rng.uniform(-4.0, 3.0, 12), rng.uniform(15.0, 25.0, 12)], axis=1)
    b = rng.uniform(0.2, 1.0, 12)
    api, model = EnergyStub(), 1  # DAC
    for level in (0, 1):
        def integrand(xx):
            e = MN.Bases(np.array([xx]), model, 2).E[0, level]
            return e * hyper[1] ** 2 * math.sqrt(2 * math.pi) / hyper[3] * float(np.sum(b * np.exp(-0.5 * (hyper[2] * (xx - X[:, 0])) ** 2)))
        lo, hi = X[:, 0].min() - 40.0 / hyper[2], X[:, 0].max() + 40.0 / hyper[2]
        knots = np.linspace(lo, hi, 81)
        ref = sum(quad(integrand, a, c, epsabs=0.0, epsrel=1e-13, limit=200)[0] for a, c in zip(knots[:-1], knots[1:]))
        got = R.potential_energy_from_gpr(api, 2, model, level, hyper, X, b)
        half = R.potential_energy_from_gpr(api, 2, model, level, hyper, X, b, step_divisor=32)
        assert abs(got - ref) <= 1e-10 * abs(ref), (level, got, ref)
        assert abs(half - got) <= 1e-10 * abs(ref), (level, half, got)


def test_restated_selection_by_hand():
    # 5 x 4 plane, |v| row-major: running sum 1, 1, 3, 3.5 | 3.5, 4.5, 4.5, 6.5 | 7, 7, 7, 7 | 7, 7, 8, 8 | 8, 8, 8, 8
    plane = np.array([[1.0, 0.0, -2.0, 0.5], [0.0, 1.0, 0.0, -2.0], [0.5, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 0.0]])
    P = RN.running_sum(plane)
    assert float(P[-1]) == 8.0
    u = np.array([0.0, 1.0, 2.0, 6.0, 7.0, 9.0, 13.0, 14.0, 15.0]) / 16.0
    cells = RN.weighted_cells(P, u)
    #           u W = 0  0.5  1.0  3.0  3.5  4.5  6.5  7.0  7.5 (exact): the first cell whose running sum EXCEEDS u W, never a cell of zero weight
    assert cells.tolist() == [0, 0, 2, 3, 5, 7, 8, 14, 14]
    assert np.all(np.abs(plane.ravel()[cells]) > 0)
    sel, K = RN.select_from_draws(cells, 4)
    assert sel.tolist() == [0, 2, 3, 5] and K == 5
    sel, K = RN.select_from_draws(cells, 6)
    assert sel.tolist() == [0, 2, 3, 5, 7, 8] and K == 7
    assert RN.uniform_cells(np.array([0.0, 0.39, 0.4, 0.999]), np.array([0.0, 0.74, 0.75, 0.999]), 5, 4).tolist() == [0, 1 * 4 + 2, 2 * 4 + 3, 19]
    # the draws: two uniforms in [0, 1) per (k, q), the same for the same seed
    u0, u1 = RN.uniforms(3, 42, 0, 1000)
    assert np.all((u0 >= 0) & (u0 < 1) & (u1 >= 0) & (u1 < 1)) and abs(u0.mean() - 0.5) < 0.05 and abs(u1.mean() - 0.5) < 0.05
    assert np.array_equal(RN.uniforms(3, 42, 500, 510)[0], u0[500:510]) and not np.array_equal(RN.uniforms(2, 42, 0, 10)[0], u0[:10])
    rho = np.zeros((2, 2, 2, 2), dtype=complex)
    rho[0, 1] = [[1 + 2j, 3 + 4j], [5 + 6j, 7 + 8j]]
    pl = RN.planes_of(rho)
    assert pl[1].tolist() == [[1, 3], [5, 7]] and pl[2].tolist() == [[2, 4], [6, 8]]  # Re above, Im below the diagonal


def test_restated_reconstruction_of_a_gaussian():
    x, p = np.linspace(-3.0, 3.0, 41), np.linspace(-12.0, 12.0, 37)
    sx, sp = 0.8, 3.0
    plane = np.exp(-((x[:, None] / sx) ** 2 + (p[None, :] / sp) ** 2) / 2.0)
    ix, ip = np.meshgrid(np.arange(0, 41, 4), np.arange(0, 37, 4), indexing="ij")
    X = np.stack([x[ix.ravel()], p[ip.ravel()]], axis=1)
    y = plane[ix.ravel(), ip.ravel()]
    hyper = np.array([1e-4, 1.0, 1.0 / sx, 1.0 / sp])
    b = np.linalg.solve(RN.train_gram(hyper, X, np.float64), y)
    mu, tol = RN.predict_plane(hyper, X, b, x, p)
    assert float(np.abs(mu - plane).max()) < 5e-3  # a Gaussian from 110 of its own samples with its own widths
    assert np.all(tol > 0) and float(tol.max()) < 1e-6
    mu2, _ = RN.predict_plane(hyper, X, b, x, p, c=1.5)
    assert float(np.abs(mu2 - 1.5 * mu).max()) < 1e-15
    # the separable product is the kernel of the summed argument
    k = RN.gram(hyper, np.stack(np.meshgrid(x, p, indexing="ij"), axis=-1).reshape(-1, 2), X)
    assert float(np.abs((k @ b.astype(RN.LD)).reshape(41, 37) - mu).max()) < 1e-15
    val, mag = RN.sums_of(mu, plane, np.full(41, 0.25), p, 2000.0, 0.1, 0.5, True)
    assert float(val[0]) == pytest.approx(float(val[4] - 2 * val[5] + (plane.astype(RN.LD) ** 2).sum()), rel=1e-9)
    assert float(val[2]) == pytest.approx(0.25 * float(val[1]), rel=1e-15) and np.all(mag >= np.abs(val))


def test_log_and_choose_layout():
    rec = dict(nlml=1.5, hyper=np.arange(16.0).reshape(4, 4), mse_before=np.arange(4.0), mse_after=np.arange(4.0) + 10,
               features=[np.array([[1.0, 2.0], [3.0, 4.0]])] * 4)
    for name in ("population", "potential", "kinetic"):
        for kind in ("exact", "grid_before", "gpr_before", "grid_after", "gpr_after"):
            rec[f"{name}_{kind}"] = np.array([0.25, 0.75])
    fields = R.log_line(2.0, rec).split()
    assert len(fields) == 1 + 1 + 16 + 8 + 2 * 15 and fields[:3] == ["2", "1.5", "0"] and fields[18:22] == ["0", "10", "1", "11"]  # main_evolve.cpp:135-178
    assert R.choose_block(rec) == " 1 2 3 4\n" * 4 + "\n"  # io.cpp:74-92
    assert R.sim_block(np.array([[[1.0, 2.0]], [[3.0, 4.0]]])) == " 1 2\n 3 4\n\n"


@pytest.fixture(scope="module")
def recon_asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "gple_recon.s"
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++20", "--offload-arch=gfx950", "--cuda-device-only", "-S", f"-I{os.path.join(ROOT, 'include')}",
                    os.path.join(CSRC, "gple_recon.hip"), "-o", str(out)], check=True, capture_output=True)
    text = out.read_text()
    return {m.group(1): m.group(0) for m in re.finditer(r"^(_ZN4gple\S+):.*?\.end_amdhsa_kernel", text, flags=re.S | re.M)}


def test_the_contraction_keeps_its_accumulators_in_registers(recon_asm):
    """no scratch in any kernel of gple_recon.hip (a spill of the MFMA accumulators costs more than any schedule gains), the contraction on the
    fp64 MFMA and inside the register budget of two workgroups per compute unit"""
    seen = 0
    for name, body in recon_asm.items():
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", body), name
        if "recon_contract_kernel" in name:
            seen += 1
            assert "v_mfma_f64_16x16x4_f64" in body or "v_mfma_f64_16x16x4f64" in body, name
            assert int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1)) <= 256, name
    assert seen == 2  # two and three levels
