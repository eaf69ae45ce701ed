"""GPU: the energy-resolved spectrum of one absorbing run (gple_dvr_spectrum; csrc/gple_dvr_spectrum.hip) against the numpy
restatement and its long-double oracle (tests/dvr_spectrum_numpy.py), against the quadratic forms of gple_dvr_flux through the sum rule, and the
driver exact.run(spectrum=...) against a numpy run of its addition.  Every test here needs the entry point: none passes without it.  Measured
ratios error / tolerance are printed before each assertion.
    psi_e columns   8 max(e_ref, eps sqrt(dim) S) in the 2-norm, S = sum_{k < K} |psi_k| from the oracle, e_ref the restatement's own distance
    density         8 max(e_ref_a, eps sqrt(dim) S^2) per (energy, channel)"""
import ctypes as C
import math

import numpy as np
import pytest

from tests import dvr_absorbing_numpy as AN
from tests import dvr_flux_numpy as FN
from tests import dvr_spectrum_numpy as SN

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
IO_DEVICE = 0x100
BAD_ARG = 1
TIMER_DVR_POWER, TIMER_DVR_SPECTRUM = 9, 11
ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
dp = lambda t: C.cast(t.data_ptr(), C.POINTER(C.c_double))
bits = lambda a: np.ascontiguousarray(a).view(np.float64)
IDS = ["%dx%d-J%d" % (shape + (J,)) for shape, J in SN.CASES]
SHAPE_IDS = lambda v: "%dx%d" % v
PERIOD = [(shape, J) for shape, J in SN.CASES if 2 ** J <= 64]
_device = {}


def _call(gpu, shape, J, energies, W="case", dt=None, **kw):
    c = FN.case(*shape)
    return gpu.dvr_spectrum(shape[0], shape[1], c["H"], c["W"] if isinstance(W, str) else W, c["dt"] if dt is None else dt, J, c["basis"], c["n_left"], c["psi0"],
                            energies, **kw)


def _spectrum(gpu, shape, J, which="general"):
    """(density (n_E, 2 num_pes), psi_e (n_E, dim), remaining) of one call per case, shared by the tests below (read only)"""
    if (shape, J, which) not in _device:
        a, Y, left = _call(gpu, shape, J, SN.case(*shape, J, which)["energies"], want_psi=True)
        a = a.reshape(len(a), -1)
        a.setflags(write=False), Y.setflags(write=False)
        _device[shape, J, which] = (a, Y, left)
    return _device[shape, J, which]


# ---- 1. no level: psi_e is psi0, the density the one-step forms of gple_dvr_flux ----------------------------------------------------------------------
@pytest.mark.parametrize("shape", AN.SHAPES, ids=SHAPE_IDS)
def test_level_zero_is_psi0_and_the_one_step_forms(gpu, shape):
    c, r = FN.case(*shape), SN.case(*shape, 0)
    a, Y, _ = _spectrum(gpu, shape, 0)
    assert Y.shape == (17, c["dim"]) and a.shape == (17, 2 * shape[0])
    assert all(np.array_equal(bits(col), bits(c["psi0"])) for col in Y)
    _, G = gpu.dvr_flux(shape[0], shape[1], c["H"], c["W"], c["dt"], 1, c["basis"], c["n_left"], want_u=False)
    one = gpu.dvr_flux_apply(shape[0], shape[1], G, c["psi0"])[0].reshape(-1)
    tol = FN.tolerance(*shape, 1) + r["density_tolerance"]
    err = np.abs(a - one[None, :])
    print("J = 0 dim = %d: max error / tolerance = %.4f" % (c["dim"], (err / tol).max()))
    assert (err <= tol).all()


# ---- 2. against the long-double oracle ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape, J", SN.CASES, ids=IDS)
def test_columns_and_densities_against_long_double_stepping(gpu, shape, J):
    r = SN.case(*shape, J)
    a, Y, _ = _spectrum(gpu, shape, J)
    dim = shape[0] * shape[1]
    assert Y.shape == (len(r["energies"]), dim) and a.shape == r["a_oracle"].shape
    err = np.sqrt(np.sum(np.abs(Y.T.astype(np.clongdouble) - r["Y_oracle"]) ** 2, axis=0)).astype(np.float64)
    print("spectrum dim = %d J = %d n_E = %d: S = %.4g, columns e_ref / floor = %.3g, device error / floor = %.3g, error / tolerance = %.4f"
          % (dim, J, len(err), r["S"], r["e_ref"].max() / (EPS * math.sqrt(dim) * r["S"]), err.max() / (EPS * math.sqrt(dim) * r["S"]),
             (err / r["column_tolerance"]).max()))
    err_a = np.abs(a - r["a_oracle"])
    print("spectrum dim = %d J = %d: density e_ref_a / (floor S) = %.3g, device error / (floor S) = %.3g, error / tolerance = %.4f"
          % (dim, J, r["e_ref_a"].max() / (EPS * math.sqrt(dim) * r["S"] ** 2), err_a.max() / (EPS * math.sqrt(dim) * r["S"] ** 2),
             (err_a / r["density_tolerance"]).max()))
    assert (err <= r["column_tolerance"]).all()
    assert (err_a <= r["density_tolerance"]).all()


# ---- 3. the sum rule, on device output alone ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape, J", PERIOD, ids=[i for v, i in zip(SN.CASES, IDS) if v in PERIOD])
def test_sum_rule_against_the_flux_forms(gpu, shape, J):
    """over the K = 2^J energies theta_m = 2 pi m / K the mean of density[m][c] is the figure of gple_dvr_flux with n_steps = K on psi0"""
    c, K = FN.case(*shape), 2 ** J
    if shape == AN.LARGE:  # no oracle densities for its 32 energies: the tolerance without e_ref_a, which asks more
        a = _call(gpu, shape, J, SN.full_period_energies(K, c["dt"]), want_remaining=False)[0].reshape(K, -1)
        density_tolerance = SN.floor_density_tolerance(*shape, J)
    else:
        a, _, _ = _spectrum(gpu, shape, J, "period")
        density_tolerance = SN.case(*shape, J, "period")["density_tolerance"].mean(axis=0)
    _, G = gpu.dvr_flux(shape[0], shape[1], c["H"], c["W"], c["dt"], K, c["basis"], c["n_left"], want_u=False)
    want = gpu.dvr_flux_apply(shape[0], shape[1], G, c["psi0"])[0].reshape(-1)
    tol = SN.flux_tolerance(*shape, K) + density_tolerance
    gap = np.abs(a.mean(axis=0) - want)
    print("sum rule dim = %d K = %d: absorbed %.6g, gap %.3g, gap / tolerance = %.4f" % (c["dim"], K, want.sum(), gap.max(), (gap / tol).max()))
    assert (gap <= tol).all()


# ---- 4. padding: a column does not depend on how many stand beside it ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", AN.SHAPES, ids=SHAPE_IDS)
def test_columns_do_not_depend_on_the_padded_width(gpu, shape):
    """within the density tolerance; the bits may differ, because the GEMM's tile choice may depend on the padded width"""
    r64, r70 = SN.case(*shape, 10), SN.case(*shape, 6)
    a64, _, _ = _spectrum(gpu, shape, 10)
    a17 = _call(gpu, shape, 10, r64["energies"][:17])[0].reshape(17, -1)
    assert len(r64["energies"]) == 64 and len(r70["energies"]) == 70
    ratio = (np.abs(a64[:17] - a17) / r64["density_tolerance"][:17]).max()
    a70, _, _ = _spectrum(gpu, shape, 6)
    one = _call(gpu, shape, 6, r70["energies"][33:34])[0].reshape(1, -1)
    ratio1 = (np.abs(a70[33:34] - one) / r70["density_tolerance"][33:34]).max()
    print("padding dim = %d: 17 of 64, difference / tolerance = %.4f; one of 70: %.4f" % (shape[0] * shape[1], ratio, ratio1))
    assert ratio <= 1.0 and ratio1 <= 1.0


# ---- 5. repeats, device pointers, outputs left out ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape, J", [((2, 23), 3), ((3, 43), 6), ((2, 96), 10)], ids=["2x23-J3", "3x43-J6", "2x96-J10"])
def test_same_bits_on_repeats_and_through_device_pointers(gpu, shape, J):
    import torch

    c, r = FN.case(*shape), SN.case(*shape, J)
    a, Y, left = _spectrum(gpu, shape, J)
    a2, Y2, left2 = _call(gpu, shape, J, r["energies"], want_psi=True)
    assert np.array_equal(bits(a2), bits(a).reshape(a2.shape)) and np.array_equal(bits(Y2), bits(Y)) and left2 == left
    a3, none, none2 = _call(gpu, shape, J, r["energies"], want_psi=False, want_remaining=False)
    assert none is None and none2 is None and np.array_equal(bits(a3), bits(a).reshape(a3.shape))
    dev = torch.device("cuda", 0)
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64).copy()).to(dev)
    n_E, dim, K = len(r["energies"]), c["dim"], 2 * shape[0]
    tH, tW, tb, tv, tE = up(c["H"]), up(c["W"]), up(c["basis"]), up(bits(c["psi0"])), up(r["energies"])
    td, tp, tl = (torch.empty(m, dtype=torch.float64, device=dev) for m in (n_E * K, n_E * 2 * dim, 1))
    torch.cuda.synchronize()
    assert gpu.lib.gple_dvr_spectrum(gpu.ctx, shape[0], shape[1], dp(tH), dp(tW), c["dt"], J, dp(tb), c["n_left"], dp(tv), dp(tE), n_E, IO_DEVICE, dp(td), dp(tp),
                                     dp(tl)) == 0
    gpu.lib.gple_ctx_synchronize(gpu.ctx)
    assert np.array_equal(td.cpu().numpy(), bits(a).reshape(-1)) and np.array_equal(tp.cpu().numpy(), bits(Y).reshape(-1)) and tl.item() == left
    bad = r["energies"].copy()
    bad[-1] = math.inf
    tE2 = up(bad)
    torch.cuda.synchronize()
    assert gpu.lib.gple_dvr_spectrum(gpu.ctx, shape[0], shape[1], dp(tH), dp(tW), c["dt"], J, dp(tb), c["n_left"], dp(tv), dp(tE2), n_E, IO_DEVICE, dp(td), None,
                                     None) == BAD_ARG


# ---- 6. what is left after the K steps -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape, J", SN.CASES, ids=IDS)
def test_remaining_against_the_propagator(gpu, shape, J):
    """|P^K psi0|^2 against |U psi0|^2 of gple_dvr_propagator(n_steps = K) + gple_dvr_apply: each state lies within the power's tolerance t of
    the stepped one, so the squared norms differ by at most (|a| + |b|) 2 t"""
    c = FN.case(*shape)
    _, _, left = _spectrum(gpu, shape, J)
    U = gpu.dvr_propagator(shape[0], shape[1], c["H"], c["W"], c["dt"], 2 ** J)
    after = gpu.dvr_apply(shape[0], shape[1], U, c["psi0"], 1)[0]
    want = float(np.vdot(after, after).real)
    tol = (math.sqrt(want) + math.sqrt(max(left, 0.0))) * 2.0 * SN.state_tolerance(*shape, J)
    print("remaining dim = %d J = %d: %.6g of %.3g, difference / tolerance = %.4f" % (c["dim"], J, left, c["norm2"], abs(left - want) / tol))
    assert abs(left - want) <= tol
    assert abs(left - SN.case(*shape, J)["remaining_oracle"]) <= tol


# ---- 7. no absorber: RK4's own loss is all there is ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", AN.SHAPES, ids=SHAPE_IDS)
def test_without_absorber_the_channels_sum_to_nothing(gpu, shape):
    """sum_c a_c(E) = |psi_e|^2 - |P psi_e|^2 lies in [0, (|H| dt)^6 / 72 |psi_e|^2] (the flux test's W = NULL bound for one step), |psi_e| <= S"""
    f = SN.free_case(*shape)
    a = _call(gpu, shape, f["J"], f["energies"], W=None, dt=f["dt"])[0].reshape(5, -1)
    tol = f["density_tolerance"].sum(axis=1)
    top = (f["normH"] * f["dt"]) ** 6 / 72.0 * f["S"] ** 2
    total = a.sum(axis=1)
    print("no absorber dim = %d: sums %s in [0, %.3g], tolerance %.3g; density error / tolerance = %.4f"
          % (shape[0] * shape[1], " ".join("%.3g" % v for v in total), top, tol.max(), (np.abs(a - f["a_oracle"]) / f["density_tolerance"]).max()))
    assert (-tol <= total).all() and (total <= top + tol).all()
    assert (np.abs(a - f["a_oracle"]) <= f["density_tolerance"]).all()


# ---- 8. arguments and the timer ----------------------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments(gpu):
    f = gpu.lib.gple_dvr_spectrum
    H, W, B = np.eye(16), np.zeros(8), np.tile(np.eye(2), (8, 1, 1))
    good = dict(num_pes=2, n=8, H=H, W=W, dt=0.1, levels=2, basis=B, n_left=4, psi0=np.ones(32), E=np.array([0.1, 0.2, 0.3]), n_E=3, a=np.zeros(12),
                Y=np.zeros(3 * 32), left=np.zeros(1))
    opt = lambda a: None if a is None else ptr(a)

    def call(**kw):
        a = {**good, **kw}
        return f(gpu.ctx, a["num_pes"], a["n"], opt(a["H"]), opt(a["W"]), a["dt"], a["levels"], opt(a["basis"]), a["n_left"], opt(a["psi0"]), opt(a["E"]), a["n_E"], 0,
                 opt(a["a"]), opt(a["Y"]), opt(a["left"]))

    assert call() == 0 and call(W=None) == 0 and call(Y=None) == 0 and call(left=None) == 0 and call(n_left=0) == 0 and call(n_left=8) == 0
    assert call(levels=0) == 0 and call(levels=30) == 0 and call(n_E=1) == 0
    many = np.full(4097, 0.1)
    assert call(E=many, n_E=4096, a=np.zeros(4 * 4096), Y=None) == 0
    for bad in (dict(num_pes=1), dict(num_pes=4, n=4), dict(n=1), dict(n=32768), dict(H=None), dict(dt=math.nan), dict(dt=math.inf),  # the propagator's
                dict(levels=31), dict(levels=-1), dict(n_E=0), dict(E=many, n_E=4097, a=np.zeros(4 * 4097), Y=None), dict(E=np.array([0.1, math.nan, 0.3])),
                dict(E=np.array([0.1, 0.2, -math.inf])), dict(basis=None), dict(psi0=None), dict(n_left=9), dict(E=None), dict(a=None)):
        assert call(**bad) == BAD_ARG, sorted(bad)


def test_spectrum_timer_counts_calls(gpu):
    c = FN.case(2, 23)
    gpu.enable_timing(True)
    try:
        before, power_before = gpu.timing(TIMER_DVR_SPECTRUM)[2], gpu.timing(TIMER_DVR_POWER)[2]
        gpu.dvr_spectrum(2, 23, c["H"], c["W"], c["dt"], 4, c["basis"], c["n_left"], c["psi0"], [0.1, 0.2])
        last, _, count = gpu.timing(TIMER_DVR_SPECTRUM)
        assert count == before + 1 and last > 0.0
        assert gpu.timing(TIMER_DVR_POWER)[2] == power_before  # the propagator's timer keeps its meaning
    finally:
        gpu.enable_timing(False)


# ---- 9. the driver ----------------------------------------------------------------------------------------------------------------------------------------------
def test_exact_run_with_spectrum_against_restated_addition(gpu, tmp_path):
    """The run of the flux file's driver test (19 outputs to t = 1152) with spectrum=16: J = 14, the 2^14 steps to t = 2048.  The device's figures
    against the numpy restatement's; no long-double stepping of 16384 steps here.  Both evaluate the same product form in fp64.  Against the
    oracle the restatement's columns lie within 11 eps sqrt(dim) S and its densities within 0.15 eps sqrt(dim) S^2 up to J = 10
    (tests/test_dvr_spectrum_host.py), the columns growing more slowly than (J + 1)^2 / 11, the densities not at all; the bound here is
    8 (J + 1) eps sqrt(dim) S^2 per figure: (J + 1) for one product's rounding per level in either evaluation, 8 as everywhere for two evaluations,
    the bilinear form and the MFMA's summation order.  S is bounded from the restated loop: |psi_k| does not grow, so the steps between two
    outputs weigh at most what the earlier output has."""
    from gaussian_process_liouville_equation_amd import exact

    res = exact.run(gpu, model=exact.SAC, num_pes=2, boundary=exact.ABSORBING, out_dir=str(tmp_path), write_phase=None, chunk_bytes=1_600_000,
                    output_time=64.0, flux=True, until_absorbed=True, spectrum=16, **AN.SMALL)
    s = res["setup"]
    _, E_ad, B = gpu.dvr_hamiltonian(2, exact.SAC, exact.REFLECTIVE, s["x"][0], s["dx"], 107, s["mass"], want_h=False)
    rows, J, left = SN.run_spectrum(s, 2, exact.SAC, B, E_ad, res["stop_time"], 16)
    assert res["stop_time"] == 1152.0 and J == res["spectrum_levels"] == 14 and res["spectrum_seconds"] > 0.0
    loop, _ = FN.run_loop(s, 2, exact.SAC, 19, B)
    norms = [math.sqrt(r["populations"].sum() / s["dx"]) for r in loop]
    S = s["output_step"] * sum(norms[:-1]) + (2 ** J - 18 * s["output_step"]) * norms[-1]
    scale = s["dx"] * s["dt"] / (2.0 * math.pi)
    tol = 8.0 * (J + 1) * EPS * math.sqrt(2 * 107) * S ** 2 * scale
    got = res["spectrum"]
    assert got.shape == (16, 5) and np.array_equal(got[:, 0], rows[:, 0])
    err = np.abs(got[:, 1:] - rows[:, 1:]).max()
    print("driver: S <= %.4g, largest rho %.4g, error %.3g, error / tolerance = %.4f" % (S, np.abs(rows[:, 1:]).max(), err, err / tol))
    assert err <= tol
    assert abs(res["spectrum_remaining"] - left) <= 1e-9  # a population: the bound of the flux file's driver test
    g = lambda v: float("%g" % v)
    text = open(tmp_path / "spectrum.txt").read()
    assert [[float(v) for v in line.split()] for line in text.splitlines()] == [[g(v) for v in row] for row in got]
    assert text == "".join(" ".join("%g" % v for v in row) + "\n" for row in got)  # the device's text is the Python writer's
    fractions = got[:, 1:] / got[:, 1:].sum(axis=1, keepdims=True)
    print("fractions at E = %.6g: %s (scattering line: %s)" % (got[8, 0], " ".join("%.4g" % v for v in fractions[8]), res["scattering_line"]))
