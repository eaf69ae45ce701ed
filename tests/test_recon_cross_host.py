"""CPU: the cross-term ARD kernel on the grid (gple_grid_reconstruct_cross, reconstruct.py with kernel="cross") — the numpy
restatement tests/recon_cross_numpy.py pinned to the oracle's explicit-point prediction, the tile-centred split against the direct sum inside
the issue's entry bound, the range rule as inequalities, the five-parameter host pieces of the driver against hand-computed values and
scipy's quadrature, the file layout, and the register budget of the new contraction kernel from the cross-compiled ISA."""
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

from gaussian_process_liouville_equation_amd import _capi, reconstruct as R
from tests import mqcl_numpy as MN
from tests import recon_cross_numpy as CN
from tests import recon_numpy as RN
from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "gaussian_process_liouville_equation_amd", "csrc")
EPS = CN.EPS


def small_case(rng, nx=21, np_=17, N=30):
    x, p = np.linspace(-3.0, 3.0, nx), np.linspace(8.0, 20.0, np_)
    X = np.stack([rng.uniform(-2.5, 2.5, N), rng.uniform(9.0, 19.0, N)], axis=1)
    y = np.exp(-((X[:, 0] - 0.3 * (X[:, 1] - 14.0)) ** 2 / 0.9 + (X[:, 1] - 14.0) ** 2 / 8.0) / 2.0) + 0.01 * rng.standard_normal(N)
    return x, p, X, y


@pytest.mark.parametrize("c", [0.35, -0.5])
def test_direct_sum_against_the_oracle(oracle, c):
    """the longdouble direct sum on the explicit points of a small grid equals oracle_nlml_cross_predict, which forms b = K^-1 y itself: the
    difference is what the two solves differ by, |k| . 50 cond eps |b|_inf (§13's bound on the weights), plus the sum's own 4 (N + 8) eps S"""
    rng = np.random.default_rng(41)
    x, p, X, y = small_case(rng)
    hyper = np.array([0.05, 0.9, 1.2, c, 0.4])
    K = CN.train_gram(hyper, X, np.float64)
    b = np.linalg.solve(K, y)
    mu, tol, centred = CN.predict_plane(hyper, X, b, x, p, threads=2)
    Xs = np.ascontiguousarray(np.stack(np.meshgrid(x, p, indexing="ij"), axis=-1).reshape(-1, 2))
    ref = oracle.nlml_predict(hyper, X, y, Xs).reshape(len(x), len(p))
    k = CN.gram(hyper, Xs, X, np.float64)
    slack = (np.abs(k).sum(axis=1) * 50 * np.linalg.cond(K) * EPS * np.abs(b).max()).reshape(mu.shape)
    err = np.abs(ref - mu.astype(np.float64))
    assert np.all(err <= tol + slack), float((err / (tol + slack)).max())
    assert float(np.abs(mu).max()) > 0.1  # a prediction, not zeros
    # the same direct sum is gram . b
    assert float(np.abs((CN.gram(hyper, Xs, X) @ b.astype(CN.LD)).reshape(mu.shape) - mu).max()) < 1e-15
    # c = 0 is the diagonal kernel of tests/recon_numpy.py
    h0 = np.array([0.05, 0.9, 1.2, 0.0, 0.4])
    mu0, _, _ = CN.predict_plane(h0, X, b, x, p, threads=2)
    mu4, _ = RN.predict_plane(h0[[0, 1, 2, 4]], X, b, x, p)
    assert float(np.abs(mu0 - mu4).max()) < 1e-15


CENTRED_CASES = [  # n, N, (a, c, b), grid steps: |a| 32 dx and |c| 32 dp up to 5.9
    (192, 50, (1.0, 0.5, 0.8), 0.05, 0.05), (192, 50, (3.0, -2.5, 0.8), 0.05, 0.05), (192, 50, (3.6875, 3.6875, 0.1), 0.05, 0.05),
    (192, 200, (0.3, -0.2, 0.4), 0.1, 0.1), (130, 37, (3.6875, -3.6875, 2.0), 0.05, 0.05)]


@pytest.mark.parametrize("n, N, acb, dx, dp", CENTRED_CASES)
def test_centred_form_against_the_direct_sum(n, N, acb, dx, dp):
    """the tile-centred split in float64 (the arithmetic of the device kernel apart from the MFMA's summation order) stays inside
    4 eps [(N + 8) S + S_A] + eps max|mu| of the longdouble direct sum in every tile, and its operand exponents below L^2 / 2"""
    rng = np.random.default_rng(n + N)
    x, p = -10.0 + dx * np.arange(n), 5.0 + dp * np.arange(n)
    X = np.stack([rng.uniform(x[0], x[-1], N), rng.uniform(p[0], p[-1], N)], axis=1)
    b = rng.standard_normal(N)
    hyper = np.array([1e-3, 0.8, *acb])
    mu, tol, centred = CN.predict_plane(hyper, X, b, x, p, c=1.25, threads=4)
    assert centred.all()
    AU, CV = CN.tile_ranges(hyper, x, p)
    got, top = CN.centred_plane(hyper, X, b, x, p, c=1.25)
    err = np.abs(got - mu.astype(np.float64))
    print(f"n={n} N={N} (a, c, b)={acb}: A_U {AU.max():.2f} C_V {CV.max():.2f} largest operand exponent {top:.2f} worst err / tol {np.max(err / tol):.3g}")
    assert np.all(err <= tol)
    assert top <= CN.LIMIT ** 2 / 2
    # in longdouble the split is the direct sum to longdouble's own rounding
    exact, _ = CN.centred_plane(hyper, X, b, x, p, c=1.25, dtype=CN.LD)
    assert np.all(np.abs(exact - mu) <= tol / 512)


def test_range_rule_on_random_tiles():
    """x exponent <= A_U^2 / 2, p exponent <= C_V^2 / 2, |cell exponent| <= A_U C_V for every point, near or far, and the three add up to -Q / 2"""
    rng = np.random.default_rng(7)
    for _ in range(200):
        a, c, b = rng.uniform(-8.0, 8.0), rng.uniform(-8.0, 8.0), rng.uniform(0.05, 4.0)
        h = 10.0 ** rng.uniform(-3.0, 0.0)
        rows, cols = rng.integers(1, 65), rng.integers(1, 65)
        x, p = rng.uniform(-10.0, 10.0) + h * np.arange(rows), rng.uniform(-30.0, 30.0) + 3.0 * h * np.arange(cols)
        xc, pc = x[min(32, rows - 1)], p[min(32, cols - 1)]
        X = np.stack([rng.uniform(-40.0, 40.0, 64), rng.uniform(-90.0, 90.0, 64)], axis=1)
        X[:8] = [xc, pc] + rng.uniform(-1.0, 1.0, (8, 2)) * [rows * h, cols * 3.0 * h]  # some points inside the tile
        u, v = x - xc, p - pc
        AU, CV = abs(a) * np.abs(u).max(), abs(c) * np.abs(v).max()
        hyper = np.array([1e-3, 1.0, a, c, b])
        ex, ep, cell = CN.split_exponents(hyper, X, u, v, xc, pc, CN.LD)
        assert float(ex.max()) <= AU * AU / 2 * (1 + 1e-12) and float(ep.max()) <= CV * CV / 2 * (1 + 1e-12)
        assert float(np.abs(cell).max()) <= AU * CV * (1 + 1e-12)
        dx, dp = x[:, None, None] - X[None, None, :, 0], p[None, :, None] - X[None, None, :, 1]
        half_q = ((a * dx + c * dp) ** 2 + (b * dp) ** 2) / 2
        total = ex[:, None, :] + ep[None, :, :] + cell[:, :, None]
        scale = np.abs(ex)[:, None, :] + np.abs(ep)[None, :, :] + np.abs(cell)[:, :, None] + half_q
        assert np.all(np.abs(total.astype(np.float64) + half_q) <= 64 * EPS * scale)
    # which tiles are centred: both ranges at most L
    x, p = np.linspace(-10.0, 10.0, 301), np.linspace(-20.0, 60.0, 130)
    hyper = np.array([1e-3, 1.0, 2.0, 0.31, 1.0])  # |a| 32 dx = 4.27; |c| 32 dp = 6.15 in the first two column tiles, |c| dp = 0.19 in the last
    assert CN.centred_tiles(hyper, x, p).tolist() == [[False, False, True]] * 5


def survey_rows(rows):
    s = np.zeros((len(rows), 8))
    for q, (mx, mn, arg) in enumerate(rows):
        s[q, 0], s[q, 1], s[q, 3] = mx, mn, arg
    return s


def test_set_initial_value_with_five_columns():
    x, p = np.linspace(-10.0, 10.0, 5), np.linspace(10.0, 30.0, 4)
    s = survey_rows([(0.5, 0.0, 2 * 4 + 1), (0.02, -0.004, 3), (0.009, -0.009, 0), (0.009, -0.02, -1)])
    lower, upper, start = R.set_initial_value(s, x, p, 2, kernel="cross")
    sigma_p = p[1] / 20.0
    big = np.finfo(np.float64).max
    assert lower.shape == upper.shape == start.shape == (4, 5)
    for q in range(4):
        assert lower[q].tolist() == [1e-8, 1e-4, 1.0 / 20.0, -big, 1.0 / 20.0]  # c unbounded both ways (gpr.cpp:143-145, 176-181)
        assert upper[q].tolist() == [1e-5, 1.0, big, big, big]
        assert start[q].tolist() == [1e-8, 1.0, 1.0 / (0.5 / sigma_p), 0.0, 1.0 / sigma_p]
    # the default is today's four columns, value for value
    l4, u4, s4 = R.set_initial_value(s, x, p, 2)
    assert l4.shape == (4, 4) and np.array_equal(l4, lower[:, [0, 1, 2, 4]]) and np.array_equal(u4, upper[:, [0, 1, 2, 4]])
    assert np.array_equal(s4, start[:, [0, 1, 2, 4]])
    with pytest.raises(ValueError):
        R.set_initial_value(s, x, p, 2, kernel="diagonal")


def test_population_and_kinetic_energy_with_five_parameters():
    hyper = np.array([1e-6, 0.5, 2.0, 0.7, 0.25])  # w_g = 0.5, W = [[2, 0], [0.7, 1 / 4]]
    X = np.array([[0.0, 3.0], [1.0, -1.0], [2.0, 2.0]])
    b = np.array([1.0, -2.0, 4.0])
    coe = 2.0 * math.pi * 0.25 / 0.5  # (2 pi) w_g^2 / (a b): the diagonal's product (gpr.cpp:750)
    assert R.population_from_gpr(hyper, b) == pytest.approx(coe * 3.0, rel=1e-15)
    # (W W^T)^-1 = [[a^2, a c], [a c, c^2 + b^2]]^-1 has a^2 / (a b)^2 = 1 / b^2 = 16 at (p, p) (gpr.cpp:896): the row vector is (25, 17, 20)
    W = np.array([[2.0, 0.0], [0.7, 0.25]])
    assert np.linalg.inv(W @ W.T)[1, 1] == pytest.approx(16.0, rel=1e-13)
    assert R.kinetic_energy_from_gpr(hyper, X, b, 2000.0) == pytest.approx(coe * (25.0 - 34.0 + 80.0) / 4000.0, rel=1e-15)
    # the integral of the kernel over phase space is what the population's coefficient says, whatever c
    from scipy.integrate import dblquad
    val = dblquad(lambda pp, xx: 0.25 * math.exp(-((2.0 * xx + 0.7 * pp) ** 2 + (0.25 * pp) ** 2) / 2.0), -30.0, 30.0, -60.0, 60.0, epsabs=1e-12, epsrel=1e-11)[0]
    assert val == pytest.approx(coe, rel=1e-8)


class EnergyStub:
    """pes_adiabatic_n of the library from the oracle's potentials (no GPU here)"""

    def pes_adiabatic_n(self, num_pes, model, x):
        return (MN.Bases(np.asarray(x), model, num_pes).E,)


@pytest.mark.parametrize("hyper", [[1e-6, 0.8, 1.0 / 0.7, 0.0, 0.25], [1e-6, 0.3, 2.5, 0.8, 1.0], [1e-6, 1.0, 0.4, -0.3, -0.05]])
def test_potential_energy_with_five_parameters_against_quad(hyper):
    """gpr.cpp:801-806 as the text reads — Characteristic(0, 1) = 0, so the marginal is w_g^2 sqrt(2 pi) / |b| exp(-(a dx)^2 / 2) — against
    scipy's quadrature of that formula; with c != 0 it is not the kernel's true marginal over p"""
    from scipy.integrate import quad
    hyper = np.array(hyper)
    wg, a, c, b = hyper[1:]
    rng = np.random.default_rng(31)
    X = np.stack([rng.uniform(-4.0, 3.0, 12), rng.uniform(15.0, 25.0, 12)], axis=1)
    w = rng.uniform(0.2, 1.0, 12)
    api, model = EnergyStub(), 1  # DAC

    def as_written(xx):  # Char2(0, 1) = 0, Char2(0, 0) = a^2, Char2(1, 1) = b^2
        return wg ** 2 * math.sqrt(2 * math.pi / (0.0 + b * b)) * float(np.sum(w * np.exp(-(xx - X[:, 0]) ** 2 * (a * a / 2.0 * (1.0 + 0.0 / (0.0 + b * b))))))

    def true_marginal(xx):  # the integral over p of w_g^2 exp(-((a dx + c dp)^2 + (b dp)^2) / 2)
        return wg ** 2 * math.sqrt(2 * math.pi / (b * b + c * c)) * float(np.sum(w * np.exp(-(a * b * (xx - X[:, 0])) ** 2 / (2.0 * (b * b + c * c)))))

    for level in (0, 1):
        energy = lambda xx: MN.Bases(np.array([xx]), model, 2).E[0, level]
        lo, hi = X[:, 0].min() - 40.0 / a, X[:, 0].max() + 40.0 / a
        knots = np.linspace(lo, hi, 81)
        ref = sum(quad(lambda xx: energy(xx) * as_written(xx), s, e, epsabs=0.0, epsrel=1e-13, limit=200)[0] for s, e in zip(knots[:-1], knots[1:]))
        got = R.potential_energy_from_gpr(api, 2, model, level, hyper, X, w)
        assert abs(got - ref) <= 1e-10 * abs(ref), (level, got, ref)
        if c == 0.0:
            assert got == R.potential_energy_from_gpr(api, 2, model, level, hyper[[0, 1, 2, 4]], X, w)  # the NOCROSS expression, bit for bit
        else:
            lo, hi = X[:, 0].min() - 40.0 * math.hypot(b, c) / abs(a * b), X[:, 0].max() + 40.0 * math.hypot(b, c) / abs(a * b)
            knots = np.linspace(lo, hi, 81)
            true = sum(quad(lambda xx: energy(xx) * true_marginal(xx), s, e, epsabs=0.0, epsrel=1e-13, limit=200)[0] for s, e in zip(knots[:-1], knots[1:]))
            assert abs(got - true) > 1e-3 * abs(true), (level, got, true)  # the reference's quirk, kept
    # the true marginal is what integrating the kernel over p gives
    xx = 0.4
    num = quad(lambda pp: float(np.sum(w * wg ** 2 * np.exp(-((a * (xx - X[:, 0]) + c * (pp - X[:, 1])) ** 2 + (b * (pp - X[:, 1])) ** 2) / 2.0))),
               X[:, 1].min() - 40.0 / abs(b), X[:, 1].max() + 40.0 / abs(b), epsabs=0.0, epsrel=1e-12, limit=400, points=sorted(X[:, 1] - (a / (b * b + c * c)) * c * (xx - X[:, 0])))[0]
    assert num == pytest.approx(true_marginal(xx), rel=1e-9)


def test_log_layout_with_five_parameters():
    rec = dict(nlml=1.5, hyper=np.arange(20.0).reshape(4, 5), mse_before=np.arange(4.0), mse_after=np.arange(4.0) + 10,
               features=[np.array([[1.0, 2.0], [3.0, 4.0]])] * 4)
    for name in ("population", "potential", "kinetic"):
        for kind in ("exact", "grid_before", "gpr_before", "grid_after", "gpr_after"):
            rec[f"{name}_{kind}"] = np.array([0.25, 0.75])
    fields = R.log_line(2.0, rec).split()
    assert len(fields) == 1 + 1 + 20 + 8 + 2 * 15 and fields[:3] == ["2", "1.5", "0"] and fields[21:26] == ["19", "0", "10", "1", "11"]


class RecordingApi:
    """the six entry points the driver calls, returning fixed shapes: which of them a kernel= choice reaches, and what the record holds"""

    def __init__(self, nx, np_):
        self.nx, self.np, self.calls = nx, np_, []

    def grid_survey(self, num_pes, model, rho, x, p, mass, dx, dp):
        s = np.zeros((4, 8))
        s[:, 0], s[:, 1], s[:, 3] = [0.5, 0.2, 0.2, 0.4], -0.1, 2 * self.np + 3
        s[[0, 3], 4], s[[0, 3], 5], s[[0, 3], 6] = [0.6, 0.4], [0.01, 0.03], [0.1, 0.07]
        return s

    def grid_select(self, num_pes, rho, x, p, q, n, seed, uniform=False):
        rng = np.random.default_rng(q)
        return np.zeros((n, 2), dtype=np.int32), np.stack([rng.uniform(-1, 1, n), rng.uniform(14, 16, n)], axis=1), rng.uniform(0.1, 0.5, n), n

    def nlml(self, xs, X, y, want_grad=True):
        self.calls.append(("nlml", len(xs)))
        xs = np.asarray(xs)
        return float(np.sum((xs - 0.5) ** 2)), (2 * (xs - 0.5) if want_grad else None)

    def _weights(self, name, width, x, X, y):
        assert len(x) == width
        self.calls.append((name, width))
        return np.full(len(y), 0.01)

    def nlml_weights(self, x, X, y):
        return self._weights("nlml_weights", 4, x, X, y)

    def nlml_cross_weights(self, x, X, y):
        return self._weights("nlml_cross_weights", 5, x, X, y)

    def _recon(self, name, width, planes, want_pred):
        assert all(len(pl[0]) == width for pl in planes)
        self.calls.append((name, width))
        sums = np.ones((4, 6))
        return (np.zeros((4, self.nx, self.np)) if want_pred else None), sums

    def grid_reconstruct(self, num_pes, model, rho, x, p, mass, dx, dp, planes, scale=None, want_pred=True):
        return self._recon("grid_reconstruct", 4, planes, want_pred)

    def grid_reconstruct_cross(self, num_pes, model, rho, x, p, mass, dx, dp, planes, scale=None, want_pred=True):
        return self._recon("grid_reconstruct_cross", 5, planes, want_pred)

    def pes_adiabatic_n(self, num_pes, model, x):
        return (MN.Bases(np.asarray(x), model, num_pes).E,)


def test_the_kernel_argument_chooses_the_entry_points(monkeypatch):
    """kernel="nocross" (the default) reaches the four-parameter entry points and gives the record its keys and shapes of before; "cross" reaches
    the five-parameter ones with the same keys and hyper (nq, 5).  The searches are stubbed: they are the library's and need the device."""
    ends = lambda lib, f, start, lower, upper, options=None: (list(np.clip(start, lower, upper)), f(list(start)), 1)
    monkeypatch.setattr(_capi, "minimize_neldermead", ends)
    monkeypatch.setattr(_capi, "minimize_auglag_eq", lambda lib, f, con, m, start, lower, upper, options=None: (list(start), f(list(start), True)[0], 1))
    assert inspect.signature(R.reconstruct).parameters["kernel"].default == "nocross"
    assert inspect.signature(R.run_mqcl).parameters["kernel"].default == "nocross"
    nx, np_ = 12, 9
    x, p = np.linspace(-3.0, 3.0, nx), np.linspace(10.0, 20.0, np_)
    rho = np.zeros((2, 2, nx, np_), dtype=complex)
    records = {}
    for kernel, width in (("nocross", 4), ("cross", 5)):
        api = RecordingApi(nx, np_)
        api.lib = None
        state = R.State(api, 2, 1, x, p, 2000.0)
        rec = R.reconstruct(api, state, rho, n_points=6, keep_pred=True, **({} if kernel == "nocross" else {"kernel": kernel}))
        records[kernel] = rec
        names = {n for n, _ in api.calls}
        assert names == ({"nlml", "nlml_weights", "grid_reconstruct"} if width == 4 else {"nlml", "nlml_cross_weights", "grid_reconstruct_cross"})
        assert all(w == width for _, w in api.calls)
        assert rec["hyper"].shape == (4, width) and rec["pred_after"].shape == (4, nx, np_) and rec["sums_before"].shape == (4, 6)
        assert len(R.log_line(0.0, rec).split()) == 2 + 4 * width + 8 + 30
    expected = {"nlml", "hyper", "evaluations", "is_small", "factors", "singular", "initial_energy", "mse_before", "mse_after", "sums_before", "sums_after",
                "survey", "cells", "features", "labels", "draws", "seconds", "pred_before", "pred_after"}
    expected |= {f"{n}_{k}" for n in ("population", "potential", "kinetic") for k in ("exact", "grid_before", "grid_after", "gpr_before", "gpr_after")}
    assert set(records["nocross"]) == expected and set(records["cross"]) == expected
    for key in expected - {"hyper", "seconds", "nlml", "evaluations", "cells", "features", "labels", "draws"}:
        assert np.shape(records["nocross"][key]) == np.shape(records["cross"][key]), key
    with pytest.raises(ValueError):
        R.reconstruct(RecordingApi(nx, np_), R.State(None, 2, 1, x, p, 2000.0), rho, kernel="both")


class CancellingApi(RecordingApi):
    """weights as an ill-conditioned fit returns them (w_d at its lower bound): 1e7 in size, cancelling to a sum of order 1"""

    def _weights(self, name, width, x, X, y):
        b = 1e7 * np.random.default_rng(len(self.calls)).standard_normal(len(y))
        b[0] += 3.0 - b.sum()
        return b


@pytest.mark.parametrize("kernel", ["nocross", "cross"])
def test_the_constraints_hold_for_weights_that_cancel(monkeypatch, kernel):
    """The numbers from the parameters after obey_conservation meet the two constraints to 1e-10 (the driver tests' bound) whatever the size of
    the weights: they are the factor times the numbers before, not a fresh sum of scaled weights, whose rounding is eps sum |b_i| = 1e-7 here."""
    ends = lambda lib, f, start, lower, upper, options=None: (list(np.clip(start, lower, upper)), f(list(start)), 1)
    monkeypatch.setattr(_capi, "minimize_neldermead", ends)
    monkeypatch.setattr(_capi, "minimize_auglag_eq", lambda lib, f, con, m, start, lower, upper, options=None: (list(start), f(list(start), True)[0], 1))
    nx, np_ = 12, 9
    x, p = np.linspace(-3.0, 3.0, nx), np.linspace(10.0, 20.0, np_)
    api = CancellingApi(nx, np_)
    api.lib = None
    rec = R.reconstruct(api, R.State(api, 2, 1, x, p, 2000.0), np.zeros((2, 2, nx, np_), dtype=complex), n_points=50, kernel=kernel)
    assert not rec["singular"] and np.all(rec["factors"][[0, 3]] != 1.0)
    assert abs(rec["population_gpr_after"].sum() - 1.0) <= 1e-10
    e_after = (rec["potential_gpr_after"] + rec["kinetic_gpr_after"]).sum()
    assert abs(e_after - rec["initial_energy"]) <= 1e-10 * abs(rec["initial_energy"])
    for name in ("population", "potential", "kinetic"):
        assert np.array_equal(rec[f"{name}_gpr_after"], rec["factors"][[0, 3]] * rec[f"{name}_gpr_before"])


def test_binding_declares_the_cross_entry_points():
    assert "nlml_cross_weights" in _capi.GPLE_SYMBOLS and "grid_reconstruct_cross" in _capi.GPLE_SYMBOLS
    assert _capi.SIGNATURES["nlml_cross_weights"] == _capi.SIGNATURES["nlml_weights"]
    assert [n for n, _ in _capi.ReconCrossPlane._fields_] == ["x", "X", "b", "N"] and _capi.ReconCrossPlane.x.size == 40
    assert callable(_capi.Api.nlml_cross_weights) and callable(_capi.Api.grid_reconstruct_cross)


@pytest.fixture(scope="module")
def recon_asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "gple_recon.s"
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++20", "--offload-arch=gfx950", "--cuda-device-only", "-S", f"-I{os.path.join(ROOT, 'include')}",
                    os.path.join(CSRC, "gple_recon.hip"), "-o", str(out)], check=True, capture_output=True)
    text = out.read_text()
    return {m.group(1): m.group(0) for m in re.finditer(r"^(_ZN4gple\S+):.*?\.end_amdhsa_kernel", text, flags=re.S | re.M)}


def test_the_cross_contraction_keeps_its_accumulators_in_registers(recon_asm):
    """no scratch in the cross-term contraction either, its products on the fp64 MFMA, inside the register and LDS budget of two workgroups per
    compute unit, and no floating-point atomics"""
    seen = 0
    for name, body in recon_asm.items():
        if "recon_cross_kernel" not in name:
            continue
        seen += 1
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", body), name
        assert "v_mfma_f64_16x16x4_f64" in body or "v_mfma_f64_16x16x4f64" in body, name
        assert int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1)) <= 256, name
        assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body).group(1)) <= 80 * 1024, name
        assert not re.search(r"atomic_(add|min|max|pk_add)_f", body), name
    assert seen == 2  # two and three levels
