"""CPU: the coupled-channel scattering solver (gple_scatter) on its numpy restatement tests/scatter_numpy.py — closed forms, the
order of the method, unitarity and reciprocity — then the binding's table and the driver scattering.run on a numpy stand-in api.

The Eckart barrier V0 sech^2(a x) transmits T = sinh^2(pi k / a) / (sinh^2(pi k / a) + cosh^2(pi / 2 sqrt(8 m V0 / a^2 - 1))); at p = 6.5,
m = 2000, V0 = 0.01, a = 1 that is 0.77324546019.  Measured with this restatement in float64: the error at N = 1000 / 2000 / 4000 on [-20, 20] is
1.149e-7, 7.19e-9, 4.49e-10 (ratios 15.98 and 16.02); |defect| at N = 6000 stays at or below 2e-13 on every case of test_unitarity."""
import functools

import numpy as np
import pytest

from gaussian_process_liouville_equation_amd import _capi
from tests import hop_numpy as HN
from tests import scatter_cases as SC
from tests import scatter_numpy as SN

MASS = SC.MASS


def test_closed_form_constants():
    cf = SC.closed_forms()
    assert abs(float(cf["eckart"]) - 0.77324546019) <= 5e-12
    assert abs(float(cf["rotated"][0]) - 0.773245460) <= 5e-10 and abs(float(cf["rotated"][1]) - 0.765355731) <= 5e-10


def test_eckart_barrier_is_fourth_order():
    """the analytic potential, so that no table's interpolation error enters: the error falls by 16 per halving of h, and the decoupled spectator
    level takes exactly nothing"""
    exact = float(SC.closed_forms()["eckart"])
    err = []
    for N in (1000, 2000, 4000):
        r = SN.march(SC.eckart, 2, MASS, -SC.BOX, SC.BOX, N, [SC.E_IN])
        prob = r["prob"][0]
        err.append(abs(prob[0, 1, 0] - exact))
        assert prob[0, 0, 1] == 0.0 and prob[0, 1, 1] == 0.0 and prob[1, 0, 0] == 0.0 and prob[1, 1, 0] == 0.0
        assert abs(r["defect"][0]).max() <= 1e-11
    print(f"eckart: error {err[0]:.4g} {err[1]:.4g} {err[2]:.4g}, ratios {err[0] / err[1]:.4g} {err[1] / err[2]:.4g}")
    assert 14.0 <= err[0] / err[1] <= 18.0 and 14.0 <= err[1] / err[2] <= 18.0
    assert err[2] < 1e-9


def test_two_channels_under_a_constant_rotation():
    """Each adiabatic channel transmits by its own closed form; nothing crosses.  The bound on the closed forms: the rule's error at N = 4000 is
    4.5e-10 for the a = 1 barrier (above) and grows with the fourth derivative, a^4 = 5 times for a = 1.5: 1e-8 holds both"""
    r = SN.march(SC.rotated, 2, MASS, -SC.BOX, SC.BOX, 4000, [SC.E_IN])
    prob, exact = r["prob"][0], SC.closed_forms()["rotated"]
    for k in range(2):
        assert abs(prob[k, 1, k] - float(exact[k])) <= 1e-8, (k, prob[k, 1, k], float(exact[k]))
        assert abs(prob[k, 0, k] - (1.0 - float(exact[k]))) <= 1e-8
        assert prob[k, 0, 1 - k] < 1e-20 and prob[k, 1, 1 - k] < 1e-20, prob[k]


UNITARITY = {"sac": (HN.SAC, 2, 40.0, 0), "dac": (HN.DAC, 2, 40.0, 0), "ecr": (HN.ECR, 2, 40.0, 0), "tsac": (HN.TSAC, 3, 30.0, 1)}


@pytest.mark.parametrize("name", list(UNITARITY))
def test_unitarity_and_reciprocity(name):
    model, N, box, surface0 = UNITARITY[name]
    pot = HN.builtin(model, N)
    eps = HN.jacobi(pot(np.array([-box]))[0])[0][0]
    p = np.array([4.0, 8.0, 10.0, 20.0, 30.0])
    r = SN.march(pot, N, MASS, -box, box, 6000, p * p / 2.0 / MASS + eps[surface0])
    prob, defect = r["prob"], r["defect"]
    open_in = ~np.isnan(defect)
    assert open_in[:, surface0].all()
    assert (np.isnan(prob).all(axis=(2, 3)) == ~open_in).all()
    print(f"{name}: largest |defect| {np.abs(defect[open_in]).max():.3g}, closed columns {(~open_in).sum()}")
    assert np.abs(defect[open_in]).max() <= 1e-11
    worst = 0.0
    for i in range(N):
        for j in range(i + 1, N):
            both = open_in[:, i] & open_in[:, j]
            if both.any():
                worst = max(worst, np.abs(prob[both, i, 0, j] - prob[both, j, 0, i]).max())
    assert worst <= 1e-11
    if name != "ecr":
        assert (~open_in).any(), "no energy with a closed upper channel: the case tests less than it says"
    assert (prob[open_in] >= 0.0).all()


def test_the_figures_of_the_prototype():
    """DESIGN.md §18's table, N = 6000 from the lower surface, box +-40 (the digits that do not depend on the box or the grid)"""
    for model, p, want in ((HN.SAC, 10.0, [4e-6, 1.1e-5, 0.844520, 0.155465]), (HN.SAC, 4.0, [0.89809, 0.0, 0.10191, 0.0]),
                           (HN.ECR, 10.0, [0.089928, 0.209911, 0.700161, 0.0]), (HN.ECR, 30.0, [0.0, 0.0, 0.569479, 0.430521])):
        pot = HN.builtin(model, 2)
        eps = HN.jacobi(pot(np.array([-40.0]))[0])[0][0]
        got = SN.march(pot, 2, MASS, -40.0, 40.0, 6000, [p * p / 2.0 / MASS + eps[0]])["prob"][0, 0].ravel()
        assert np.abs(got - np.array(want)).max() <= 6e-6, (model, p, got)


# ---- fails without the feature ---------------------------------------------------------------------------------------------------------------------
def test_the_binding_declares_gple_scatter():
    assert "scatter" in _capi.GPLE_SYMBOLS
    assert _capi.TIMER_SCATTER == 21


@functools.lru_cache(maxsize=None)
def driver_run():
    from gaussian_process_liouville_equation_amd import scattering
    api = SN.NumpyScatterApi()
    momenta = np.array([4.0, 6.0, 8.0, 10.0, 12.0])
    return scattering, api, momenta, scattering.run(api, model=scattering.SAC, num_pes=2, momenta=momenta, x_left=-8.0, x_right=8.0, richardson=True)


def test_driver_energy_map_and_default_grid():
    scattering, api, momenta, r = driver_run()
    pot = HN.builtin(HN.SAC, 2)
    ends = np.linalg.eigvalsh(np.stack([pot(np.array([-8.0]))[0][0], pot(np.array([8.0]))[0][0]]))
    assert np.allclose(r["energies"], momenta ** 2 / 2.0 / MASS + ends[0, 0], rtol=1e-15, atol=0)
    assert np.array_equal(r["head"], momenta)
    N = r["n_steps"]
    k_max = np.sqrt(2.0 * MASS * (r["energies"].max() - ends.min()))
    assert k_max * 16.0 / N <= 0.1 < k_max * 16.0 / (N - 1)
    assert api.calls == [(N, 5), (2 * N, 5)]
    by_energy = scattering.run(SN.NumpyScatterApi(), model=scattering.SAC, energies=r["energies"], x_left=-8.0, x_right=8.0, n_steps=200)
    assert np.allclose(by_energy["momenta"], momenta, rtol=1e-12)
    with pytest.raises(ValueError):
        scattering.run(api, model=scattering.SAC, x_left=-8.0, x_right=8.0)


def test_driver_richardson_combination():
    _, _, _, r = driver_run()
    pot, N = HN.builtin(HN.SAC, 2), r["n_steps"]
    coarse = SN.march(pot, 2, MASS, -8.0, 8.0, N, r["energies"])
    fine = SN.march(pot, 2, MASS, -8.0, 8.0, 2 * N, r["energies"])
    assert np.array_equal(r["prob"], (16.0 * fine["prob"] - coarse["prob"]) / 15.0, equal_nan=True)
    assert np.array_equal(r["scattered"], r["prob"][:, 0]) and r["scattered"].shape == (5, 2, 2)
    assert np.array_equal(r["error"], np.abs(fine["prob"] - coarse["prob"])[:, 0])
    assert np.array_equal(r["defect"], fine["defect"][:, 0])
    # the extrapolation is the better figure: it lies within the error estimate of the fine grid's
    assert (np.abs(r["scattered"] - fine["prob"][:, 0]) <= r["error"]).all()


def test_driver_writes_smatrix_txt(tmp_path):
    scattering, _, momenta, r = driver_run()
    again = scattering.run(SN.NumpyScatterApi(), model=scattering.SAC, momenta=momenta, x_left=-8.0, x_right=8.0, n_steps=r["n_steps"], out_dir=str(tmp_path))
    rows = np.loadtxt(tmp_path / "smatrix.txt")
    assert rows.shape == (5, 1 + 4 + 1)
    want = np.concatenate([momenta[:, None], again["scattered"].reshape(5, 4), again["defect"][:, None]], axis=1)
    assert np.allclose(rows, want, rtol=5e-6, atol=0)
    assert open(tmp_path / "smatrix.txt").read() == "".join(again["lines"])
    assert again["lines"][0] == " ".join("%g" % v for v in want[0]) + "\n"
    dac = scattering.run(SN.NumpyScatterApi(), model=scattering.DAC, momenta=[10.0], x_left=-8.0, x_right=8.0, n_steps=200)
    assert dac["head"][0] == np.log(10.0 ** 2 / 2.0 / MASS)


def test_packet_line_is_the_weighted_sum():
    scattering, _, _, _ = driver_run()
    kw = dict(model=scattering.SAC, num_pes=2, surface0=0, x_left=-8.0, x_right=8.0, n_steps=400)
    line = scattering.packet_line(SN.NumpyScatterApi(), p0=10.0, sigma_p=0.5, n_points=33, **kw)
    p = np.linspace(7.0, 13.0, 33)
    w = np.exp(-0.5 * ((p - 10.0) / 0.5) ** 2)
    cols = scattering.run(SN.NumpyScatterApi(), momenta=p, **kw)["scattered"]
    direct = sum(w[k] * cols[k] for k in range(33)) / w.sum()
    assert line.shape == (2, 2) and np.abs(line - direct).max() <= 1e-15
    assert abs(line.sum() - 1.0) <= 1e-11
    with pytest.raises(ValueError):
        scattering.packet_line(SN.NumpyScatterApi(), p0=2.0, sigma_p=0.5, **kw)
