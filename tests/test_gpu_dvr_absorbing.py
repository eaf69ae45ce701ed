"""GPU: the absorbing boundary of the exact DVR dynamics (gple_dvr_absorber, gple_dvr_propagator, gple_dvr_apply; csrc/gple_dvr_power.hip)
against the numpy restatement and its long-double RK4 stepping (tests/dvr_absorbing_numpy.py), and the driver exact.run(boundary=ABSORBING)
against a numpy run of its loop.  Measured ratios error / tolerance are printed before each assertion."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import dvr_absorbing_numpy as AN
from tests import dvr_numpy as DN

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
IO_DEVICE = 0x100
BAD_ARG = 1
ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
dp = lambda t: C.cast(t.data_ptr(), C.POINTER(C.c_double))


def _device_h(gpu, c):
    """H as gple_dvr_hamiltonian returns it for a case of the restatement (reflective: the absorbing run's H)"""
    return gpu.dvr_hamiltonian(c["num_pes"], AN.MODEL[c["num_pes"]], DN.REFLECTIVE, c["x_first"], AN.DX, c["n"], AN.MASS)


# ---- 1. the absorber --------------------------------------------------------------------------------------------------------------------------
def test_absorber_against_restatement(gpu):
    from gaussian_process_liouville_equation_amd import exact

    grids = [(c["x_first"], AN.DX, c["n"], AN.MASS, c["xmin"], c["xmax"], AN.LENGTH) for c in (AN.case(*shape) for shape in AN.SHAPES)]
    s = exact.setup(0.0, boundary=exact.ABSORBING)  # the default grid: 1935 points, seven of them absorbing on either side
    grids.append((s["x"][0], s["dx"], s["n_grids"], s["mass"], s["xmin"], s["xmax"], s["absorbing_length"]))
    for x_first, dx, n, mass, xmin, xmax, length in grids:
        W = gpu.dvr_absorber(x_first, dx, n, mass, xmin, xmax, length)
        x = DN.grid(x_first, dx, n)
        inside, pref, a, b, c2 = AN.absorber_terms(x, mass, xmin, xmax, length)
        ref = AN.absorber(x, mass, xmin, xmax, length)
        tol = 8 * EPS * pref * (a + b + c2)
        print("absorber n = %d: max error / tolerance = %.3f" % (n, (np.abs(W - ref) / tol).max()))
        assert (np.abs(W - ref) <= tol).all()
        edge = (x == xmin) | (x == xmax)
        assert edge.sum() == 2 and not W[inside | edge].any()  # exact zeros inside the box and at both edges
        assert (W[~(inside | edge)] > 0).all()


def test_absorber_invalid_arguments_and_device_pointer(gpu):
    import torch

    f = gpu.lib.gple_dvr_absorber
    W = np.empty(32)
    good = dict(x_first=-1.0, dx=AN.DX, n=32, mass=2000.0, xmin=-0.75, xmax=0.75, length=AN.LENGTH)
    call = lambda out=W, **kw: f(gpu.ctx, *[{**good, **kw}[k] for k in ("x_first", "dx", "n", "mass", "xmin", "xmax", "length")], 0, None if out is None else ptr(out))
    assert call() == 0
    for bad in (dict(length=0.0), dict(length=-1.0), dict(length=math.nan), dict(xmin=0.75), dict(xmin=1.0), dict(xmax=math.inf), dict(mass=0.0),
                dict(dx=0.0), dict(n=1), dict(x_first=math.nan), dict(xmin=math.nan), dict(mass=math.inf)):
        assert call(**bad) == BAD_ARG, bad
    assert call(out=None) == BAD_ARG
    # the pole lies one length outside the box: an end point at (to rounding: beyond) it is refused on either side, one just inside is not
    assert call(xmin=-1.0 + 0.25, length=0.25) == BAD_ARG and call(xmin=-1.0 + 0.25, length=0.2500001) == 0
    assert call(xmax=-1.0 + 31 * AN.DX - 0.25, length=0.25) == BAD_ARG and call(xmax=-1.0 + 31 * AN.DX - 0.25, length=0.2500001) == 0
    assert call(xmin=-0.5, length=0.4) == BAD_ARG  # beyond the pole on the left
    t = torch.empty(32, dtype=torch.float64, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    assert f(gpu.ctx, -1.0, AN.DX, 32, 2000.0, -0.75, 0.75, AN.LENGTH, IO_DEVICE, dp(t)) == 0
    gpu.lib.gple_ctx_synchronize(gpu.ctx)
    assert np.array_equal(t.cpu().numpy(), gpu.dvr_absorber(-1.0, AN.DX, 32, 2000.0, -0.75, 0.75, AN.LENGTH))


# ---- 2. one step: Horner on the device against the standard product bound ------------------------------------------------------------------------
@pytest.mark.parametrize("num_pes, n", AN.SHAPES)
def test_one_step_propagator(gpu, num_pes, n):
    c = AN.case(num_pes, n)
    U = gpu.dvr_propagator(num_pes, n, c["H"], c["W"], c["dt"], 1)
    A = AN.generator(c["H"], c["W"], num_pes, c["dt"])
    ld = (c["dim"] + 63) // 64 * 64
    bound = 4 * ld * EPS * AN.p4(np.abs(A))  # P4 evaluated on |A|: every path of the Horner form, with absolute values
    err = np.abs(U - AN.p4(A))
    print("one step dim = %d: max error / bound = %.4f" % (c["dim"], (err / bound.real).max()))
    assert (err <= bound.real).all()
    assert np.array_equal(U, U.T)
    # without an absorber the same holds, and the real plane's diagonal then carries no first-order term
    U0 = gpu.dvr_propagator(num_pes, n, c["H"], None, c["dt"], 1)
    A0 = AN.generator(c["H"], None, num_pes, c["dt"])
    assert (np.abs(U0 - AN.p4(A0)) <= (4 * ld * EPS * AN.p4(np.abs(A0))).real).all()


# ---- 3. powers against long-double stepping ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", AN.POWERS)
@pytest.mark.parametrize("num_pes, n", AN.SHAPES)
def test_powers_against_long_double_stepping(gpu, num_pes, n, s):
    c = AN.case(num_pes, n)
    U = gpu.dvr_propagator(num_pes, n, c["H"], c["W"], c["dt"], s)
    assert np.array_equal(U, U.T)  # exactly symmetric: row- and column-major readers agree
    err = float(np.linalg.norm((U @ c["psi0"]).astype(np.clongdouble) - c["states"][s]))
    tol = AN.tolerance(num_pes, n, s)
    print("power dim = %d s = %d: e_ref = %.3g, device error = %.3g, error / tolerance = %.4f" % (c["dim"], s, AN.reference_error(num_pes, n, s), err, err / tol))
    assert err <= tol


def test_powers_on_the_64_tile_gemm(gpu):
    """The shapes above have at most nine 64-tiles, where every product runs the split-k GEMM; runs at the driver's defaults (ld = 3904) take the
    64 x 64 kernel with lower tiles only and beta = 1.  dim 1062 (ld 1088 = 17 tiles a side: past the split-k threshold, no multiple of 128) takes
    that kernel; s = 37 has squarings and multiplications.  The same tolerance as above."""
    num_pes, n = AN.LARGE
    s = AN.LARGE_POWERS[0]
    c = AN.case(num_pes, n)
    U = gpu.dvr_propagator(num_pes, n, c["H"], c["W"], c["dt"], s)
    assert np.array_equal(U, U.T)
    err = float(np.linalg.norm((U @ c["psi0"]).astype(np.clongdouble) - c["states"][s]))
    tol = AN.tolerance(num_pes, n, s)
    print("power dim = %d s = %d: e_ref = %.3g, device error = %.3g, error / tolerance = %.4f" % (c["dim"], s, AN.reference_error(num_pes, n, s), err, err / tol))
    assert err <= tol
    # and one step, entrywise, on the same kernel
    U1 = gpu.dvr_propagator(num_pes, n, c["H"], c["W"], c["dt"], 1)
    A = AN.generator(c["H"], c["W"], num_pes, c["dt"])
    bound = 4 * 1088 * EPS * AN.p4(np.abs(A))
    print("one step dim = %d: max error / bound = %.4f" % (c["dim"], (np.abs(U1 - AN.p4(A)) / bound).max()))
    assert (np.abs(U1 - AN.p4(A)) <= bound).all()


# ---- 4. no absorber: the spectral propagator at s dt -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_pes, n", AN.SHAPES)
def test_without_absorber_against_spectral_propagation(gpu, num_pes, n):
    """RK4's truncation for a Hermitian H: |exp(-i th) - P4(-i th)| <= th^5 / 120 per step and eigenvalue (the alternating Taylor remainder), so
    s steps differ from exp(-i H s dt) psi0 by at most s (|H| dt)^5 / 120 |psi0|; dt is chosen to make that 1e-9 |psi0|"""
    c = AN.case(num_pes, n)  # its grid and packet; H comes from the device, and no W
    s = 37
    H, _, _ = _device_h(gpu, c)
    lam, V = np.linalg.eigh(H)
    normH = float(np.abs(lam).max())
    dt = (1e-9 * 120.0 / s) ** 0.2 / normH
    psi0, nrm = c["psi0"], float(np.linalg.norm(c["psi0"]))
    U = gpu.dvr_propagator(num_pes, n, H, None, dt, s)
    got = gpu.dvr_apply(num_pes, n, U, psi0, 1)[0]
    want = gpu.dvr_propagate(num_pes, n, V, lam, psi0, np.array([s * dt]))[0]
    stepped = AN.rk4_states(H, None, num_pes, dt, psi0, (s,))[s]
    e_ref = float(np.linalg.norm((AN.power(AN.p4(AN.generator(H, None, num_pes, dt)), s) @ psi0).astype(np.clongdouble) - stepped))
    bound = s * (normH * dt) ** 5 / 120.0 * nrm + 8.0 * max(e_ref, EPS * math.sqrt(c["dim"]) * nrm)
    err = float(np.linalg.norm(got - want))
    print("no absorber dim = %d: truncation bound %.3g, error %.3g, error / bound = %.4f" % (c["dim"], bound, err, err / bound))
    assert err <= bound


# ---- 5. apply -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_pes, n", AN.SHAPES)
def test_apply(gpu, num_pes, n):
    import torch

    from gaussian_process_liouville_equation_amd import exact

    c = AN.case(num_pes, n)
    dim, psi0, nrm = c["dim"], c["psi0"], float(np.linalg.norm(c["psi0"]))
    _, _, B = _device_h(gpu, c)
    U = gpu.dvr_propagator(num_pes, n, c["H"], c["W"], c["dt"], 37)
    psi = gpu.dvr_apply(num_pes, n, U, psi0, 5)
    # numpy powers of the downloaded U: both sides round one matrix-vector product per application, |fl(U v) - U v| <= dim eps | |U| |v| |,
    # and U is a contraction, so the k-th states differ by at most 2 k dim eps | |U| |_2 |psi0|
    gamma = 2 * dim * EPS * float(np.linalg.norm(np.abs(U), 2)) * nrm
    v = psi0
    for k in range(5):
        v = U @ v
        err = float(np.linalg.norm(psi[k] - v))
        print("apply dim = %d k = %d: error / bound = %.4f" % (dim, k + 1, err / ((k + 1) * gamma)))
        assert err <= (k + 1) * gamma
    bits = lambda a: np.ascontiguousarray(a).view(np.float64)
    # continued from its last state, repeated, with U left on the device, and through device pointers: the same bits
    head = gpu.dvr_apply(num_pes, n, U, psi0, 3)
    tail = gpu.dvr_apply(num_pes, n, U, head[-1], 2)
    assert np.array_equal(bits(np.concatenate([head, tail])), bits(psi))
    assert np.array_equal(bits(gpu.dvr_apply(num_pes, n, U, psi0, 5)), bits(psi))
    Ud = gpu.dvr_propagator(num_pes, n, c["H"], c["W"], c["dt"], 37, device_out=True)
    assert tuple(Ud.shape) == (2, dim, dim) and np.array_equal(Ud.cpu().numpy(), np.stack([U.real, U.imag]))
    assert np.array_equal(bits(gpu.dvr_apply(num_pes, n, Ud, psi0, 5)), bits(psi))
    for wrong in (Ud[0], Ud.cpu(), Ud.float(), Ud.transpose(1, 2)):  # one plane, a host tensor, another type, a strided view
        with pytest.raises(ValueError):
            gpu.dvr_apply(num_pes, n, wrong, psi0, 1)
    dev = torch.device("cuda", 0)
    tv = torch.from_numpy(bits(psi0).copy()).to(dev)
    tout = torch.empty(5 * 2 * dim, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    assert gpu.lib.gple_dvr_apply(gpu.ctx, num_pes, n, dp(Ud), dp(tv), 5, None, IO_DEVICE, dp(tout)) == 0
    gpu.lib.gple_ctx_synchronize(gpu.ctx)
    assert np.array_equal(tout.cpu().numpy(), bits(psi).reshape(-1))
    # the adiabatic output is basis^T psi per grid point: num_pes products and sums per entry
    ad = gpu.dvr_apply(num_pes, n, U, psi0, 5, basis=B)
    ref = exact.to_adiabatic(psi, B)
    mag = np.abs(psi).reshape(5, num_pes, n).sum(axis=1)  # sum_j |psi_j(a)| >= sum_j |b_jk| |psi_j(a)|
    assert (np.abs(ad - ref).reshape(5, num_pes, n) <= 2 * (num_pes + 1) * EPS * mag[:, None, :]).all()


def test_propagator_and_apply_invalid_arguments(gpu):
    fp, fa = gpu.lib.gple_dvr_propagator, gpu.lib.gple_dvr_apply
    H, W, U, v, out = np.eye(16), np.zeros(8), np.zeros(2 * 16 * 16), np.zeros(32), np.zeros(32)
    assert fp(gpu.ctx, 2, 8, ptr(H), ptr(W), 0.1, 1, 0, ptr(U)) == 0
    for num_pes, n, dt, steps in ((1, 8, 0.1, 1), (4, 4, 0.1, 1), (2, 1, 0.1, 1), (2, 8, math.nan, 1), (2, 8, math.inf, 1), (2, 8, 0.1, 0), (2, 8, 0.1, (1 << 30) + 1)):
        assert fp(gpu.ctx, num_pes, n, ptr(H), ptr(W), dt, steps, 0, ptr(U)) == BAD_ARG, (num_pes, n, dt, steps)
    assert fp(gpu.ctx, 2, 32768, ptr(H), ptr(W), 0.1, 1, 0, ptr(U)) == BAD_ARG  # dim 65536 > 65472: refused before anything is read
    assert fp(gpu.ctx, 2, 8, None, ptr(W), 0.1, 1, 0, ptr(U)) == BAD_ARG and fp(gpu.ctx, 2, 8, ptr(H), ptr(W), 0.1, 1, 0, None) == BAD_ARG
    assert fa(gpu.ctx, 2, 8, ptr(U), ptr(v), 1, None, 0, ptr(out)) == 0
    assert fa(gpu.ctx, 2, 8, ptr(U), ptr(v), 0, None, 0, None) == 0  # nothing to do
    for num_pes, n, T in ((1, 8, 1), (4, 4, 1), (2, 1, 1), (2, 8, 4097)):
        assert fa(gpu.ctx, num_pes, n, ptr(U), ptr(v), T, None, 0, ptr(out)) == BAD_ARG, (num_pes, n, T)
    assert fa(gpu.ctx, 2, 8, None, ptr(v), 1, None, 0, ptr(out)) == BAD_ARG and fa(gpu.ctx, 2, 8, ptr(U), None, 1, None, 0, ptr(out)) == BAD_ARG


def test_power_timer_counts_calls(gpu):
    c = AN.case(2, 23)
    gpu.enable_timing(True)
    try:
        before = gpu.timing(9)[2]
        gpu.dvr_propagator(2, 23, c["H"], c["W"], c["dt"], 5)
        last, _, count = gpu.timing(9)
        assert count == before + 1 and last > 0.0
    finally:
        gpu.enable_timing(False)


# ---- 6. absorption: Tully's single avoided crossing leaves the small box ---------------------------------------------------------------------------
def _populations(psi, basis, dx):
    n, num_pes = basis.shape[0], basis.shape[1]
    ad = np.einsum("ajk,ja->ka", basis, psi.reshape(num_pes, n))
    return (np.abs(ad) ** 2).sum(axis=1) * dx


def test_absorption_of_the_sac_packet(gpu):
    """Every state of the twelve applications within the tolerance of the powers test, 8 max(e_ref, eps sqrt(dim) |psi0|), unscaled: every
    application is a contraction and the state shrinks, so the first application's e_ref (the numpy power of 1600 steps against the long-double
    stepping) serves all twelve.  "The populations never increase" is asserted on the total: the surfaces exchange population through the
    coupling, so a single surface's population may and does rise (3.6e-4 -> 8.1e-4 on the lower one in the restatement), while W only
    removes.  That reading is recorded here and in DESIGN.md §11 (tests paragraph of the absorbing boundary)."""
    a = AN.absorption_case()
    n, K, dx, psi0 = a["n"], AN.ABSORPTION_APPLICATIONS, AN.DX, a["psi0"]
    total = lambda v: float(np.vdot(v, v).real * dx)
    ref_totals = np.array([total(v) for v in a["states"]])
    print("restatement totals:", " ".join("%.3g" % t for t in ref_totals))
    assert (ref_totals[8:] < AN.PPL_LIM).all() and ref_totals[0] > 0.99  # below PplLim from the ninth application on
    W = gpu.dvr_absorber(a["x"][0], dx, n, AN.MASS, AN.SMALL["xmin"], AN.SMALL["xmax"], AN.LENGTH)
    assert np.abs(W - a["W"]).max() <= 8 * EPS * a["W"].max()
    U = gpu.dvr_propagator(2, n, a["H"], W, AN.DT, AN.ABSORPTION_STEPS, device_out=True)
    psi = gpu.dvr_apply(2, n, U, psi0, K)
    totals = np.array([total(psi0)] + [total(v) for v in psi])
    assert (np.diff(totals) <= 0).all()
    nrm = float(np.linalg.norm(psi0))
    tol = 8.0 * max(a["e_ref"], EPS * math.sqrt(2 * n) * nrm)
    for k in range(K):
        err = float(np.linalg.norm(psi[k] - a["states"][k]))
        print("absorption k = %d: total %.3g, error %.3g, error / tolerance = %.4f" % (k + 1, totals[k + 1], err, err / tol))
        assert err <= tol
        # populations: | |u|^2 - |v|^2 | dx <= (|u| + |v|) |u - v| dx
        moved = np.abs(_populations(psi[k], a["basis"], dx) - _populations(a["states"][k], a["basis"], dx)).max()
        assert moved <= (math.sqrt(totals[k + 1] / dx) + math.sqrt(ref_totals[k] / dx)) * tol * dx + 4 * EPS * ref_totals[k]


# ---- 7. the driver --------------------------------------------------------------------------------------------------------------------------------
def test_exact_run_absorbing_against_restated_loop(gpu, tmp_path):
    from gaussian_process_liouville_equation_amd import exact

    res = exact.run(gpu, model=exact.SAC, num_pes=2, boundary=exact.ABSORBING, max_outputs=8, out_dir=str(tmp_path), write_phase="text", chunk_bytes=1_600_000,
                    output_time=64.0, **AN.SMALL)
    s = res["setup"]
    assert (s["n_grids"], s["n_absorbing"], s["dt"], s["halvings"], s["output_step"]) == (107, 5, 0.125, 0, 512)
    assert res["eigh_seconds"] == 0.0 and res["propagator_seconds"] > 0.0
    _, _, B = gpu.dvr_hamiltonian(2, exact.SAC, exact.REFLECTIVE, s["x"][0], s["dx"], 107, s["mass"], want_h=False)
    ref, stop = AN.run_loop(s, 2, exact.SAC, 8, B)
    # the packet's <x> passes -x0 = 1.5 between t = 256 and t = 320: both loops stop there, at the sixth output
    assert len(res["records"]) == len(ref) == 6 and stop == "OUT" and res["stop"] == "GET OUT OF INTERACTING REGION, STOP EVOLVING AT 320"
    for a, b in zip(res["records"], ref):
        assert a["t"] == b["t"]
        assert np.abs(a["populations"] - b["populations"]).max() <= 1e-9
        for k in ("E", "x"):
            assert abs(a[k] - b[k]) <= 1e-9 * max(1.0, abs(b[k])), (k, a[k], b[k])
    # the files, parsed back: every number is the "%g" text of the record's value
    g = lambda v: float("%g" % v)
    assert [float(v) for v in open(tmp_path / "t.txt").read().split()] == [r["t"] for r in ref] == [64.0 * k for k in range(6)]
    assert [float(v) for v in open(tmp_path / "x.txt").read().split()] == [g(v) for v in s["x"]]
    rows = [[float(v) for v in line.split()] for line in open(tmp_path / "averages.txt").read().splitlines()]
    assert len(rows) == 6 and all(len(r) == 9 for r in rows)
    for row, a, b in zip(rows, res["records"], ref):
        assert row[:6] == [g(a["t"]), g(a["E"]), g(a["x"]), g(a["p"]), g(a["populations"][0]), g(a["populations"][1])]
        assert row[6:] == [g(v) for v in a["phase_averages"]]
        assert abs(row[4] - b["populations"][0]) <= 1e-5 * b["populations"][0] + 1e-9  # six significant digits of the restatement's value
    psi_rows = [[float(v) for v in line.split()] for line in open(tmp_path / "psi.txt").read().splitlines()]
    assert len(psi_rows) == 6 and all(len(r) == 214 for r in psi_rows)
    for row, b in zip(psi_rows, ref):
        dens = np.abs(b["psi_adia"]) ** 2
        assert np.abs(np.array(row) - dens).max() <= 1e-5 * dens.max()
    assert len(open(tmp_path / "phase.txt").read().split("\n")) == 5 * 6 + 1
    assert len(res["final_line"].split()) == 3
