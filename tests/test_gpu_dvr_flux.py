"""GPU: what the absorber took (gple_dvr_flux, gple_dvr_flux_apply; csrc/gple_dvr_flux.hip) against the numpy restatement and
its long-double oracle (tests/dvr_flux_numpy.py), and the driver exact.run(flux=True, until_absorbed=True) against a numpy run of its loop.
Every test here needs the two entry points: none passes without them.  Measured ratios error / tolerance are printed before each assertion."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import dvr_absorbing_numpy as AN
from tests import dvr_flux_numpy as FN

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
IO_DEVICE = 0x100
BAD_ARG = 1
TIMER_DVR_FLUX = 10
ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
dp = lambda t: C.cast(t.data_ptr(), C.POINTER(C.c_double))
bits = lambda a: np.ascontiguousarray(a).view(np.float64)
CASES = [(shape, s) for shape in AN.SHAPES for s in FN.POWERS] + [(AN.LARGE, AN.LARGE_POWERS[0])]
IDS = ["%dx%d-s%d" % (shape + (s,)) for shape, s in CASES]
_device = {}


def _flux(gpu, shape, s):
    """(U, G) of one gple_dvr_flux call per case, shared by the tests below (host arrays, read only)"""
    if (shape, s) not in _device:
        c = FN.case(*shape)
        U, G = gpu.dvr_flux(shape[0], shape[1], c["H"], c["W"], c["dt"], s, c["basis"], c["n_left"])
        U.setflags(write=False), G.setflags(write=False)
        _device[shape, s] = (U, G)
    return _device[shape, s]


# ---- 1. U is the propagator's, bit for bit; G does not depend on whether U is asked for ---------------------------------------------------------
@pytest.mark.parametrize("shape, s", CASES, ids=IDS)
def test_u_has_the_bits_of_the_propagator(gpu, shape, s):
    c = FN.case(*shape)
    U, G = _flux(gpu, shape, s)
    assert np.array_equal(bits(U), bits(gpu.dvr_propagator(shape[0], shape[1], c["H"], c["W"], c["dt"], s)))
    none, G2 = gpu.dvr_flux(shape[0], shape[1], c["H"], c["W"], c["dt"], s, c["basis"], c["n_left"], want_u=False)
    assert none is None and np.array_equal(bits(G2), bits(G))


# ---- 2. structure ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape, s", CASES, ids=IDS)
def test_every_channel_is_exactly_hermitian(gpu, shape, s):
    _, G = _flux(gpu, shape, s)
    assert G.shape == (2 * shape[0], shape[0] * shape[1], shape[0] * shape[1])
    for g in G:
        assert np.array_equal(g.real, g.real.T) and np.array_equal(g.imag, -g.imag.T)
        assert not np.diag(g.imag).any() and not np.signbit(np.diag(g.imag)).any()  # exact (positive) zeros


# ---- 3. one step: D_c entrywise --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", AN.SHAPES + [AN.LARGE], ids=lambda v: "%dx%d" % v)
def test_one_step_against_the_split_of_the_loss(gpu, shape):
    """G_c of one step is D_c = (Pi_c L + L Pi_c) / 2 with L = I - conj(P) P.  With B = I + |P|^T |P| and |P| = P4(|A|), entrywise
        |fl(L) - L| <= k ld eps B,   k = 13 = 2 + 2 + 8 + 1:
    2 for the device's product conj(P) P (four real GEMMs, two of them summed into each plane: 2 ld terms per entry), 2 for numpy's own product on
    the reference side, 8 for the error the device's P carries from its Horner form, 4 ld eps P4(|A|) (test_one_step_propagator of the sibling
    file) in either factor, 1 for the subtraction from I and for the roundings of the mix.  D_c mixes num_pes entries of L along a row and along
    a column with the weights b b' of the projector, so the bound goes through the same mix with |Pi_c|: k ld eps (|Pi_c| B + B |Pi_c|) / 2."""
    num_pes, n = shape
    c = FN.case(num_pes, n)
    _, G = _flux(gpu, shape, 1)
    A = AN.generator(c["H"], c["W"], num_pes, c["dt"])
    D = FN.channels(FN.loss(AN.p4(A)), c["basis"], c["n_left"])
    absP = AN.p4(np.abs(A)).real
    B = np.eye(c["dim"]) + absP.T @ absP
    ld = (c["dim"] + 63) // 64 * 64
    for ch in range(2 * num_pes):
        PB = FN.project(np.abs(c["basis"]), c["n_left"], ch, B)
        bound = 13 * ld * EPS * 0.5 * (PB + PB.T)
        err = np.abs(G[ch] - D[ch])
        where = bound > 0
        print("one step dim = %d channel %d: max error / bound = %.4f" % (c["dim"], ch, (err[where] / bound[where]).max()))
        assert (err <= bound).all()


# ---- 4. powers against the long-double oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape, s", [v for v in CASES if v[1] != 1], ids=[i for v, i in zip(CASES, IDS) if v[1] != 1])
def test_quadratic_forms_against_long_double_stepping(gpu, shape, s):
    c = FN.case(*shape)
    _, G = _flux(gpu, shape, s)
    got, tol = FN.forms(G, c["psi0"]), FN.tolerance(*shape, s)
    err = np.abs(got - c["absorbed"][s])
    print("flux dim = %d s = %d: absorbed %.6g of %.3g, e_ref = %.3g, device error = %.3g, error / tolerance = %.4f"
          % (c["dim"], s, got.sum(), c["norm2"], FN.e_ref(*shape, s), err.max(), err.max() / tol))
    assert (err <= tol).all()


# ---- 5. the channels add up to the norm loss, on device output alone ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape, s", [v for v in CASES if v[1] != 1], ids=[i for v, i in zip(CASES, IDS) if v[1] != 1])
def test_channels_add_up_to_the_norm_loss(gpu, shape, s):
    c = FN.case(*shape)
    U, G = _flux(gpu, shape, s)
    taken = gpu.dvr_flux_apply(shape[0], shape[1], G, c["psi0"])[0]
    after = gpu.dvr_apply(shape[0], shape[1], U, c["psi0"], 1)[0]
    gap = taken.sum() + np.vdot(after, after).real - c["norm2"]
    tol = 2 * shape[0] * FN.tolerance(*shape, s)
    print("identity dim = %d s = %d: gap %.3g, gap / tolerance = %.4f" % (c["dim"], s, gap, abs(gap) / tol))
    assert abs(gap) <= tol


# ---- 6. no absorber: RK4's own loss is all there is -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_pes, n", AN.SHAPES)
def test_without_absorber_only_the_loss_of_rk4(gpu, num_pes, n):
    """|P4(-i th)|^2 = 1 - th^6 / 72 + th^8 / 576 <= 1 for th <= sqrt(8): a step loses at most (|H| dt)^6 / 72 of the norm and gains nothing, so
    the channels sum into [0, s (|H| dt)^6 / 72 |psi0|^2]; dt as in test_without_absorber_against_spectral_propagation of the sibling file"""
    c = FN.case(num_pes, n)
    s, H, psi0 = 37, c["H"], c["psi0"]
    normH = float(np.abs(np.linalg.eigvalsh(H)).max())
    dt = (1e-9 * 120.0 / s) ** 0.2 / normH
    _, G = gpu.dvr_flux(num_pes, n, H, None, dt, s, c["basis"], c["n_left"], want_u=False)
    taken = gpu.dvr_flux_apply(num_pes, n, G, psi0)[0]
    _, Gn = FN.flux_matrices(H, None, num_pes, dt, s, c["basis"], c["n_left"])
    stepped = np.asarray(FN.oracle(H, None, num_pes, dt, psi0, (s,), c["basis"], c["n_left"])[s][0], dtype=np.float64)
    e_ref = float(np.abs(FN.forms(Gn, psi0) - stepped).max())
    tol = 2 * num_pes * 8.0 * max(e_ref, EPS * math.sqrt(c["dim"]) * c["norm2"])
    top = s * (normH * dt) ** 6 / 72.0 * c["norm2"]
    print("no absorber dim = %d: sum %.3g in [0, %.3g], oracle %.3g, tolerance %.3g" % (c["dim"], taken.sum(), top, stepped.sum(), tol))
    assert -tol <= taken.sum() <= top + tol
    assert (np.abs(FN.forms(G, psi0) - stepped) <= tol / (2 * num_pes)).all()


# ---- 7. the application ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_pes, n", AN.SHAPES)
def test_apply_against_numpy_forms_and_its_own_bits(gpu, num_pes, n):
    import torch

    c = FN.case(num_pes, n)
    dim, psi0, K = c["dim"], c["psi0"], 2 * num_pes
    _, G = _flux(gpu, (num_pes, n), 37)
    states = np.stack([c["states"][s].astype(np.complex128) for s in (2, 3, 37)] + [psi0, c["states"][1000].astype(np.complex128)])  # psi0 fourth of five
    got = gpu.dvr_flux_apply(num_pes, n, G, states)
    assert got.shape == (5, 2, num_pes)
    for t, v in enumerate(states):
        want = FN.forms(G, v)
        tol = 4 * dim * EPS * np.array([np.abs(v) @ (np.abs(g) @ np.abs(v)) for g in G])
        err = np.abs(got[t].reshape(-1) - want)
        print("flux apply dim = %d state %d: max error / tolerance = %.4f" % (dim, t, (err / tol).max()))
        assert (err <= tol).all()
    # alone, repeated, in a call that takes more than one pass over G (70 states: two chunks, the last group of four not full), with G left on
    # the device and through device pointers: the same bits
    alone = gpu.dvr_flux_apply(num_pes, n, G, psi0)
    assert alone.shape == (1, 2, num_pes) and np.array_equal(bits(alone[0]), bits(got[3]))
    assert np.array_equal(bits(gpu.dvr_flux_apply(num_pes, n, G, states)), bits(got))
    many = np.concatenate([np.tile(states, (13, 1)), states[:4], psi0[None, :]])  # psi0 at 3 + 5 j, and last of 70
    got70 = gpu.dvr_flux_apply(num_pes, n, G, many)
    assert np.array_equal(bits(got70[:65]), bits(np.tile(got, (13, 1, 1)))) and np.array_equal(bits(got70[69]), bits(got[3]))
    _, Gd = gpu.dvr_flux(num_pes, n, c["H"], c["W"], c["dt"], 37, c["basis"], c["n_left"], device_out=True, want_u=False)
    assert tuple(Gd.shape) == (K, 2, dim, dim) and np.array_equal(Gd.cpu().numpy(), np.stack([G.real, G.imag], axis=1))
    assert np.array_equal(bits(gpu.dvr_flux_apply(num_pes, n, Gd, states)), bits(got))
    for wrong in (Gd[0], Gd.cpu(), Gd.float(), Gd.transpose(2, 3)):
        with pytest.raises(ValueError):
            gpu.dvr_flux_apply(num_pes, n, wrong, psi0)
    dev = torch.device("cuda", 0)
    tv = torch.from_numpy(bits(states).copy()).to(dev)
    tout = torch.empty(5 * K, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    assert gpu.lib.gple_dvr_flux_apply(gpu.ctx, num_pes, n, dp(Gd), dp(tv), 5, IO_DEVICE, dp(tout)) == 0
    gpu.lib.gple_ctx_synchronize(gpu.ctx)
    assert np.array_equal(tout.cpu().numpy(), bits(got).reshape(-1))


# ---- 8. Tully's single avoided crossing leaves the small box: reflection and transmission per surface ----------------------------------------------
def test_scattering_of_the_sac_packet(gpu):
    a = FN.absorption_case()
    n, K, dx, psi0 = a["n"], AN.ABSORPTION_APPLICATIONS, AN.DX, a["psi0"]
    total = lambda v: float(np.vdot(v, v).real * dx)
    U, G = gpu.dvr_flux(2, n, a["H"], a["W"], AN.DT, AN.ABSORPTION_STEPS, a["basis"], a["n_left"], device_out=True)
    psi = gpu.dvr_apply(2, n, U, psi0, K)
    before = np.concatenate([psi0[None, :], psi[:-1]])  # the state each application starts from
    cumulative = np.cumsum(gpu.dvr_flux_apply(2, n, G, before).reshape(K, 4), axis=0) * dx
    for k in range(K):
        gap = cumulative[k].sum() + total(psi[k]) - total(psi0)
        print("scattering k = %d: absorbed %s, left %.3g, gap %.3g" % (k + 1, " ".join("%.6g" % v for v in cumulative[k]), total(psi[k]), gap))
        assert abs(gap) <= 1e-11
    # the figures of the restatement's own states through the device's G against the restatement's G: the tolerance of test 4 per application,
    # in populations (times dx); every state is smaller than psi0, whose e_ref serves all twelve
    ref_before = np.concatenate([psi0[None, :], a["states"][:-1]])
    device = np.cumsum(gpu.dvr_flux_apply(2, n, G, ref_before).reshape(K, 4), axis=0) * dx
    tol = 8.0 * max(a["e_ref_flux"], EPS * math.sqrt(2 * n) * float(np.vdot(psi0, psi0).real)) * dx
    for k in range(K):
        err = np.abs(device[k] - a["cumulative"][k] * dx).max()
        print("scattering k = %d: error %.3g, error / tolerance = %.4f" % (k + 1, err, err / ((k + 1) * tol)))
        assert err <= (k + 1) * tol
    print("reflected %.6g %.6g, transmitted %.6g %.6g, left %.3g (restatement: %s)"
          % (*cumulative[-1], total(psi[-1]), " ".join("%.6g" % (v * dx) for v in a["cumulative"][-1])))


# ---- 9. arguments and the timer --------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments(gpu):
    ff, fa = gpu.lib.gple_dvr_flux, gpu.lib.gple_dvr_flux_apply
    H, W, B = np.eye(16), np.zeros(8), np.tile(np.eye(2), (8, 1, 1))
    U, G, v, out = np.zeros(2 * 16 * 16), np.zeros(4 * 2 * 16 * 16), np.ones(32), np.zeros(4)
    good = dict(num_pes=2, n=8, H=H, W=W, dt=0.1, steps=1, basis=B, n_left=4, U=U, G=G)
    order = ("num_pes", "n", "H", "W", "dt", "steps", "basis", "n_left")
    opt = lambda a: None if a is None else ptr(a)

    def call(**kw):
        a = {**good, **kw}
        return ff(gpu.ctx, a["num_pes"], a["n"], opt(a["H"]), opt(a["W"]), a["dt"], a["steps"], opt(a["basis"]), a["n_left"], 0, opt(a["U"]), opt(a["G"]))

    assert call() == 0 and call(W=None) == 0 and call(U=None) == 0 and call(n_left=0) == 0 and call(n_left=8) == 0
    for bad in (dict(basis=None), dict(n_left=9), dict(num_pes=1), dict(num_pes=4, n=4), dict(steps=0), dict(steps=(1 << 30) + 1), dict(dt=math.nan),
                dict(dt=math.inf), dict(G=None), dict(H=None), dict(n=1), dict(n=32768)):
        assert call(**bad) == BAD_ARG, bad
    assert fa(gpu.ctx, 2, 8, ptr(G), ptr(v), 1, 0, ptr(out)) == 0
    big = np.zeros(2 * 16 * 4097)
    for num_pes, n, T in ((2, 8, 0), (2, 8, 4097), (1, 8, 1), (4, 4, 1), (2, 1, 1)):
        assert fa(gpu.ctx, num_pes, n, ptr(G), ptr(big), T, 0, ptr(out)) == BAD_ARG, (num_pes, n, T)
    assert fa(gpu.ctx, 2, 8, None, ptr(v), 1, 0, ptr(out)) == BAD_ARG and fa(gpu.ctx, 2, 8, ptr(G), None, 1, 0, ptr(out)) == BAD_ARG
    assert fa(gpu.ctx, 2, 8, ptr(G), ptr(v), 1, 0, None) == BAD_ARG


def test_flux_timer_counts_calls(gpu):
    c = FN.case(2, 23)
    gpu.enable_timing(True)
    try:
        before, power_before = gpu.timing(TIMER_DVR_FLUX)[2], gpu.timing(9)[2]
        gpu.dvr_flux(2, 23, c["H"], c["W"], c["dt"], 5, c["basis"], c["n_left"])
        last, _, count = gpu.timing(TIMER_DVR_FLUX)
        assert count == before + 1 and last > 0.0
        assert gpu.timing(9)[2] == power_before  # the propagator's timer keeps its meaning
    finally:
        gpu.enable_timing(False)


# ---- 10. the driver ------------------------------------------------------------------------------------------------------------------------------
def test_exact_run_with_flux_against_restated_loop(gpu, tmp_path):
    from gaussian_process_liouville_equation_amd import exact

    """The step list of the small box ends at t = 1152, before the slow reflected part (1.3e-3) has left: both loops run all 19 outputs, past the
    sixth, where the reference's criteria stop (the sibling file's driver test).  The PplLim ending itself is tested on scripted states in
    tests/test_dvr_flux_host.py."""
    res = exact.run(gpu, model=exact.SAC, num_pes=2, boundary=exact.ABSORBING, out_dir=str(tmp_path), write_phase=None, chunk_bytes=1_600_000,
                    output_time=64.0, flux=True, until_absorbed=True, **AN.SMALL)
    s = res["setup"]
    assert (s["n_grids"], s["dt"], s["output_step"]) == (107, 0.125, 512) and res["flux_seconds"] > 0.0
    _, _, B = gpu.dvr_hamiltonian(2, exact.SAC, exact.REFLECTIVE, s["x"][0], s["dx"], 107, s["mass"], want_h=False)
    ref, stop = FN.run_loop(s, 2, exact.SAC, 19, B)
    assert stop is None and res["stop"] is None and len(res["records"]) == len(ref) == 19
    for a, b in zip(res["records"], ref):
        assert a["t"] == b["t"] and a["absorbed"].shape == (2, 2)
        assert np.abs(a["populations"] - b["populations"]).max() <= 1e-9 and np.abs(a["absorbed"] - b["absorbed"]).max() <= 1e-9
        assert abs(a["absorbed"].sum() + a["populations"].sum() - res["records"][0]["populations"].sum()) <= 1e-11
    g = lambda v: float("%g" % v)
    rows = [[float(v) for v in line.split()] for line in open(tmp_path / "absorbed.txt").read().splitlines()]
    assert len(rows) == len(ref) and all(len(r) == 6 for r in rows)
    for row, a in zip(rows, res["records"]):
        assert row == [g(a["t"])] + [g(v) for v in a["absorbed"].ravel()] + [g(a["populations"].sum())]
    last = res["records"][-1]
    assert np.array_equal(res["absorbed"], last["absorbed"])
    assert res["scattering_line"] == " ".join("%g" % v for v in [s["p0"], *last["absorbed"].ravel(), last["populations"].sum()])
    assert res["scattering_line"].split()[:1] == res["final_line"].split()[:1]
    print("scattering line:", res["scattering_line"])
