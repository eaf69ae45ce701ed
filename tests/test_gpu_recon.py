"""GPU: reconstruction of a gridded density with the NLML GP (gple_nlml_weights, gple_grid_survey, gple_grid_select, gple_grid_reconstruct;
csrc/gple_recon.hip) against the longdouble restatement tests/recon_numpy.py, and the driver reconstruct.py on a synthetic
two-level state.  eps = 2^-53 throughout; every bound is the one the arithmetic allows (summation order, exp's relative error), none is measured."""
import math

import numpy as np
import pytest

from gaussian_process_liouville_equation_amd import _capi, reconstruct
from tests import mqcl_numpy as MN
from tests import recon_numpy as RN

pytestmark = pytest.mark.gpu
EPS = RN.EPS
MASS = 2000.0
SX, SP = 0.7, 4.0  # widths of the synthetic packets


def grid(nx, np_, xmin=-10.0, xmax=10.0, p0=20.0, half=40.0):
    i, j = np.arange(nx, dtype=np.float64), np.arange(np_, dtype=np.float64)
    x = (xmin * (nx - 1 - i) + xmax * i) / (nx - 1)
    p = ((p0 - half) * (np_ - 1 - j) + (p0 + half) * j) / (np_ - 1)
    return x, p, (x[-1] - x[0]) / nx, (p[-1] - p[0]) / np_  # dx, dp as main_evolve.cpp:23


def packets(num_pes, x, p):
    """a Hermitian state of Gaussian packets: rho_aa at different places, rho_ab their geometric mean with a phase"""
    rho = np.zeros((num_pes, num_pes, len(x), len(p)), dtype=np.complex128)
    centres = [(-2.0, 20.0), (1.5, 14.0), (3.0, 27.0)]
    weights = [0.6, 0.3, 0.1]
    g = [w * np.exp(-(((x[:, None] - cx) / SX) ** 2 + ((p[None, :] - cp) / SP) ** 2) / 2.0) / (2 * math.pi * SX * SP)
         for (cx, cp), w in zip(centres, weights)]
    for a in range(num_pes):
        rho[a, a] = g[a]
        for b in range(a + 1, num_pes):
            rho[a, b] = np.sqrt(g[a] * g[b]) * np.exp(0.5j * (x[:, None] - centres[a][0]))
            rho[b, a] = np.conj(rho[a, b])
    return rho


def random_hermitian(num_pes, nx, np_, rng):
    r = rng.standard_normal((num_pes, num_pes, nx, np_)) + 1j * rng.standard_normal((num_pes, num_pes, nx, np_))
    r = 0.5 * (r + np.conj(np.swapaxes(r, 0, 1)))
    for a in range(num_pes):
        r[a, a] = r[a, a].real
    return np.ascontiguousarray(r)


def evolved_state(gpu, num_pes, model, n, steps=50):
    """an MQCLE state `steps` Trotter steps after the packets, in the adiabatic representation"""
    x, p, _, _ = grid(n, n)
    rho = gpu.mqcl_transform(num_pes, model, x, packets(num_pes, x, p), MN.ADIABATIC, MN.DIABATIC)
    rho = gpu.mqcl_evolve(num_pes, model, x, p, rho, MASS, x[-1] - x[0], p[-1] - p[0], 0.5, steps)
    return gpu.mqcl_observe(num_pes, model, x, p, rho, MASS, 1.0, 1.0)[0]


def training_points(plane, x, p, N, rng):
    """N distinct cells drawn with probability |v| (numpy's generator: the selection has its own test)"""
    w = np.abs(plane).ravel()
    cells = np.sort(rng.choice(w.size, size=N, replace=False, p=w / w.sum()))
    X = np.stack([x[cells // len(p)], p[cells % len(p)]], axis=1)
    return np.ascontiguousarray(X), plane.ravel()[cells].copy()


HYPER = np.array([1e-3, 0.8, 1.0 / SX, 1.0 / SP])  # (w_d, w_g, a_x, a_p)


# ---- 5. weights -------------------------------------------------------------------------------------------------------------------------
def solve_longdouble(K, y):
    """Cholesky solve in longdouble (numpy.linalg has none): the yardstick for the figures printed below, not for an assertion"""
    A, n = K.astype(RN.LD).copy(), len(y)
    for j in range(n):
        A[j, j] = np.sqrt(A[j, j] - A[j, :j] @ A[j, :j])
        A[j + 1:, j] = (A[j + 1:, j] - A[j + 1:, :j] @ A[j, :j]) / A[j, j]
    z = y.astype(RN.LD).copy()
    for j in range(n):
        z[j] = (z[j] - A[j, :j] @ z[:j]) / A[j, j]
    for j in range(n - 1, -1, -1):
        z[j] = (z[j] - A[j + 1:, j] @ z[j + 1:]) / A[j, j]
    return z


@pytest.mark.parametrize("N", [150, 1024])
def test_weights(gpu, N):
    """b = K^-1 y against numpy.linalg.solve within 50 cond eps |b|_inf on the data and hyper-parameters of test_nlml_at_baseline_sizes, the
    test the bound is modelled on (noise 0.05, cond 4e4 ... 3e5; measured 0.02 and 0.09 of the bound).  On a grid-selected set with noise 1e-3
    (cond 4e7 at N = 150, 2e8 at N = 1024) the figures against a longdouble solve are printed without an assertion: on the MI355X the device
    is 111 and 192 cond eps |b|_inf away from it, numpy.linalg.solve 0.33 and 0.44 — the NLML path multiplies by the explicit inverse factor,
    b = T^T (T y), whose forward error carries |K^-1| |y| where a triangular solve carries |b|."""
    from tests import parity
    X, y, _ = parity.synthetic_real(N, 4, 4400 + N)
    hyper = np.array([0.05, 1.3, 1.0 / 0.7086, 1.0 / 0.7056])
    b = gpu.nlml_weights(hyper, X, y)
    K = RN.train_gram(hyper, X, np.float64)
    ref = np.linalg.solve(K, y)
    cond = np.linalg.cond(K)
    err, bound = np.abs(b - ref).max(), 50 * cond * EPS * np.abs(ref).max()
    print(f"weights N={N}: cond {cond:.3g} err {err:.3g} bound {bound:.3g}")
    assert err <= bound
    assert np.array_equal(b, gpu.nlml_weights(hyper, X, y))
    # the prediction of the same kernel is gram(Xs, X) b with these very weights
    Xs = np.ascontiguousarray(np.stack(np.meshgrid(np.linspace(-12.0, -8.0, 14), np.linspace(12.0, 16.0, 14), indexing="ij"), axis=-1).reshape(-1, 2))
    k = RN.gram(hyper, Xs, X)
    mean = gpu.nlml_predict(hyper, X, y, Xs)
    tol = 4 * (N + 8) * EPS * (np.abs(k) * np.abs(b)[None, :]).sum(axis=1).astype(np.float64)
    diff = np.abs(mean - (k @ b.astype(RN.LD)).astype(np.float64))
    print(f"  predict: worst err / tol {np.max(diff / tol):.3g}")
    assert np.all(diff <= tol)
    for bad in (dict(x=[1e-3, 0.8, np.nan, 1.0]), dict(X=X[:0], y=y[:0])):
        with pytest.raises(_capi.GpleError):
            gpu.nlml_weights(bad.get("x", hyper), bad.get("X", X), bad.get("y", y))
    # figures only: the ill-conditioned set of the reconstruction tests
    x, p, _, _ = grid(257, 257)
    Xg, yg = training_points(RN.planes_of(packets(2, x, p))[0], x, p, N, np.random.default_rng(500 + N))
    Kg = RN.train_gram(HYPER, Xg, np.float64)
    bg, ng, lg = gpu.nlml_weights(HYPER, Xg, yg), np.linalg.solve(Kg, yg), solve_longdouble(RN.train_gram(HYPER, Xg), yg)
    unit = np.linalg.cond(Kg) * EPS * float(np.abs(lg).max())
    print(f"  grid set, cond {np.linalg.cond(Kg):.3g}: device - longdouble {float(np.abs(bg - lg).max()) / unit:.3g}, numpy - longdouble "
          f"{float(np.abs(ng - lg).max()) / unit:.3g}, device - numpy {np.abs(bg - ng).max() / unit:.3g}  (units of cond eps |b|_inf)")


# ---- 6. survey --------------------------------------------------------------------------------------------------------------------------
def check_survey(gpu, num_pes, model, rho, x, p, dx, dp):
    out = gpu.grid_survey(num_pes, model, rho, x, p, MASS, dx, dp)
    val, mag = RN.survey(rho, x, p, MASS, dx, dp, MN.Bases(x, model, num_pes).E)
    assert np.array_equal(out[:, :2], val[:, :2].astype(np.float64)) and np.array_equal(out[:, 3], val[:, 3].astype(np.float64))
    assert np.all(out[:, 7] == 0.0)
    for k in (2, 4, 5, 6):
        err, tol = np.abs(out[:, k] - val[:, k]).astype(np.float64), (len(x) * len(p) * EPS * mag[:, k]).astype(np.float64)
        print(f"survey {num_pes} levels {len(x)}x{len(p)} field {gpu.SURVEY_FIELDS[k]}: worst err / tol {np.max(err / np.maximum(tol, 1e-300)):.3g}")
        assert np.all(err <= tol), (k, err, tol)
    assert np.array_equal(out, gpu.grid_survey(num_pes, model, rho, x, p, MASS, dx, dp))


@pytest.mark.parametrize("num_pes, nx, np_", [(2, 47, 96), (3, 47, 96), (2, 257, 257), (3, 257, 257), (2, 961, 961)])
def test_survey(gpu, num_pes, nx, np_):
    x, p, dx, dp = grid(nx, np_)
    model = 1
    rng = np.random.default_rng(600 + nx + num_pes)
    check_survey(gpu, num_pes, model, random_hermitian(num_pes, nx, np_, rng), x, p, dx, dp)
    rho = evolved_state(gpu, num_pes, model, nx) if nx == np_ else packets(num_pes, x, p)
    check_survey(gpu, num_pes, model, rho, x, p, dx, dp)
    neg = -np.abs(random_hermitian(num_pes, nx, np_, rng).real) - 1.0  # nothing above 0: no maximum index
    assert np.all(gpu.grid_survey(num_pes, model, neg.astype(np.complex128), x, p, MASS, dx, dp)[:, 3] == -1.0)


def test_survey_bad_arguments(gpu):
    x, p, dx, dp = grid(8, 9)
    rho = packets(2, x, p)
    for kw in (dict(mass=0.0), dict(dx=np.inf), dict(model=7)):
        with pytest.raises(_capi.GpleError):
            gpu.grid_survey(2, kw.get("model", 1), rho, x, p, kw.get("mass", MASS), kw.get("dx", dx), dp)


# ---- 7. selection -----------------------------------------------------------------------------------------------------------------------
def check_weighted_selection(gpu, num_pes, rho, x, p, q, n_select, seed):
    cells, X, y, K = gpu.grid_select(num_pes, rho, x, p, q, n_select, seed)
    plane = RN.planes_of(rho)[q]
    flat = cells[:, 0].astype(np.int64) * len(p) + cells[:, 1]
    assert np.all(np.diff(flat) > 0)  # ascending (ix, ip), distinct
    assert np.array_equal(X[:, 0], x[cells[:, 0]]) and np.array_equal(X[:, 1], p[cells[:, 1]]) and np.array_equal(y, plane.ravel()[flat])
    assert np.all(np.abs(y) > 0.0)  # never a cell of zero weight
    P = RN.running_sum(plane)
    tau = RN.LD(plane.size * EPS) * P[-1]
    u, _ = RN.uniforms(q, seed, 0, K)
    uk = u.astype(RN.LD) * P[-1]
    # draw k may select every cell c with P(c - 1) - tau <= u_k < P(c) + tau
    cmin, cmax = np.searchsorted(P, uk - tau, side="right"), np.searchsorted(P, uk + tau, side="right")
    cmax = np.minimum(cmax, plane.size - 1)
    lo, hi = np.searchsorted(flat, cmin, side="left"), np.searchsorted(flat, cmax, side="right")
    assert np.all(hi > lo), "a draw among the first K has no selected cell in its interval"
    covered = np.zeros(n_select, dtype=bool)
    for a, b in zip(lo, hi):
        covered[a:b] = True
    assert covered.all(), "a selected cell that no draw among the first K can have produced"
    ref_draws = RN.weighted_cells(P, u)
    ambiguous = int(np.count_nonzero(cmin != cmax))
    print(f"selection plane {q}: K = {K}, {ambiguous} draws with more than one admissible cell")
    if ambiguous == 0:
        ref, K_ref = RN.select_from_draws(ref_draws, n_select)
        assert K == K_ref and np.array_equal(flat, ref)
        assert len(set(ref_draws[:K - 1].tolist())) == n_select - 1  # K is minimal
    return cells, X, y, K


def test_selection_weighted(gpu):
    n = 257
    x, p, _, _ = grid(n, n)
    rho = evolved_state(gpu, 2, 1, n)
    for q in range(4):
        first = check_weighted_selection(gpu, 2, rho, x, p, q, 200, seed=20240607)
        again = gpu.grid_select(2, rho, x, p, q, 200, 20240607)
        assert all(np.array_equal(a, b) for a, b in zip(first[:3], again[:3])) and first[3] == again[3]
        other = gpu.grid_select(2, rho, x, p, q, 200, 20240608)
        assert not np.array_equal(first[0], other[0])
    rho3 = packets(3, *grid(47, 96)[:2])
    x3, p3, _, _ = grid(47, 96)
    for q in (0, 5, 7, 8):
        check_weighted_selection(gpu, 3, rho3, x3, p3, q, 37, seed=99)


def test_selection_device_pointers(gpu):
    import torch
    x, p, _, _ = grid(47, 96)
    rho = packets(2, x, p)
    host = gpu.grid_select(2, rho, x, p, 1, 37, 5)
    dev = gpu.grid_select(2, torch.from_numpy(rho).cuda(), torch.from_numpy(x).cuda(), torch.from_numpy(p).cuda(), 1, 37, 5)
    gpu.synchronize()
    assert all(np.array_equal(h, d.cpu().numpy()) for h, d in zip(host[:3], dev[:3])) and host[3] == dev[3]


def test_selection_uniform(gpu):
    x, p, _, _ = grid(47, 96)
    rho = packets(2, x, p)
    for q, seed in ((0, 1), (3, 77)):
        cells, X, y, K = gpu.grid_select(2, rho, x, p, q, 300, seed, uniform=True)
        u, u2 = RN.uniforms(q, seed, 0, 4096)
        ref, K_ref = RN.select_from_draws(RN.uniform_cells(u, u2, len(x), len(p)), 300)
        assert K == K_ref and np.array_equal(cells[:, 0].astype(np.int64) * len(p) + cells[:, 1], ref)
        assert np.array_equal(y, RN.planes_of(rho)[q].ravel()[ref]) and np.array_equal(X[:, 0], x[cells[:, 0]])


def test_selection_bad_arguments(gpu):
    x, p, _, _ = grid(8, 8)
    rho = np.zeros((2, 2, 8, 8), dtype=np.complex128)
    rho[0, 0, 2:4, 3:6] = 1.0  # six cells of non-zero weight
    assert gpu.grid_select(2, rho, x, p, 0, 6, 3)[3] >= 6
    with pytest.raises(_capi.GpleError):
        gpu.grid_select(2, rho, x, p, 0, 7, 3)   # more points than cells of non-zero weight
    with pytest.raises(_capi.GpleError):
        gpu.grid_select(2, rho, x, p, 1, 1, 3)   # a plane without weight
    with pytest.raises(_capi.GpleError):
        gpu.grid_select(2, rho, x, p, 0, 65, 3, uniform=True)  # more points than cells
    with pytest.raises(_capi.GpleError):
        gpu.grid_select(2, rho, x, p, 4, 3, 3)   # no such plane
    assert gpu.grid_select(2, rho, x, p, 0, 64, 3, uniform=True)[3] >= 64


# ---- 8. reconstruction ------------------------------------------------------------------------------------------------------------------
def fitted_planes(gpu, rho, x, p, N, empty, rng):
    planes_v, planes = RN.planes_of(rho), []
    for q, v in enumerate(planes_v):
        if q in empty:
            planes.append(None)
            continue
        X, y = training_points(v, x, p, N, rng)
        hyper = HYPER * np.array([1.0, 1.0 + 0.1 * q, 1.0 + 0.05 * q, 1.0 - 0.03 * q])
        planes.append((hyper, X, gpu.nlml_weights(hyper, X, y), y))
    return planes_v, planes


RECON_CASES = [(2, 47, 96, 37, (), False), (3, 47, 96, 37, (5,), True), (2, 257, 257, 200, (2,), True), (3, 257, 257, 200, (), False),
               (2, 961, 961, 200, (), True), (2, 961, 961, 1024, (1, 2), False), (3, 961, 961, 200, (2, 3, 5, 6, 7), True)]


@pytest.mark.parametrize("num_pes, nx, np_, N, empty, scaled", RECON_CASES)
def test_reconstruct(gpu, num_pes, nx, np_, N, empty, scaled):
    import torch
    x, p, dx, dp = grid(nx, np_)
    model = 1
    rho = packets(num_pes, x, p)
    rng = np.random.default_rng(800 + nx + N + num_pes)
    planes_v, planes = fitted_planes(gpu, rho, x, p, N, empty, rng)
    nq = num_pes * num_pes
    scale = np.array([1.0 + 0.3 * math.cos(1.0 + q) for q in range(nq)]) if scaled else None
    args = [None if pl is None else pl[:3] for pl in planes]
    pred, sums = gpu.grid_reconstruct(num_pes, model, rho, x, p, MASS, dx, dp, args, scale)
    energies = MN.Bases(x, model, num_pes).E
    for q in range(nq):
        c = 1.0 if scale is None else scale[q]
        diag = RN.is_diagonal(q, num_pes)
        if planes[q] is None:
            assert np.all(pred[q] == 0.0)
            mu, tol = np.zeros((nx, np_), dtype=RN.LD), np.zeros((nx, np_))
        else:
            hyper, X, b, _ = planes[q]
            mu, tol = RN.predict_plane(hyper, X, b, x, p, c)
            err = np.abs(pred[q] - mu).astype(np.float64)
            print(f"reconstruct {num_pes} levels {nx}x{np_} N={N} plane {q}: worst err / tol {np.max(err / tol):.3g}, max|mu| {float(np.abs(mu).max()):.3g}")
            assert np.all(err <= tol)
        val, mag = RN.sums_of(mu, planes_v[q], energies[:, q // num_pes], p, MASS, dx, dp, diag)
        stol = RN.sums_tolerance(mu, planes_v[q], tol, energies[:, q // num_pes], p, MASS, dx, dp, diag) + nx * np_ * EPS * mag.astype(np.float64)
        serr = np.abs(sums[q] - val).astype(np.float64)
        print(f"  sums plane {q}: err / tol {serr / np.maximum(stol, 1e-300)}")
        assert np.all(serr <= stol), (q, serr, stol)
        if not diag:
            assert np.all(sums[q, 1:4] == 0.0)
    # the same bits again, without pred, and through device pointers
    pred2, sums2 = gpu.grid_reconstruct(num_pes, model, rho, x, p, MASS, dx, dp, args, scale)
    assert np.array_equal(pred, pred2) and np.array_equal(sums, sums2)
    assert np.array_equal(sums, gpu.grid_reconstruct(num_pes, model, rho, x, p, MASS, dx, dp, args, scale, want_pred=False)[1])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dargs = [None if a is None else (a[0], t(a[1]), t(a[2])) for a in args]
    dpred, dsums = gpu.grid_reconstruct(num_pes, model, t(rho), t(x), t(p), MASS, dx, dp, dargs, scale)
    gpu.synchronize()
    assert np.array_equal(pred, dpred.cpu().numpy()) and np.array_equal(sums, dsums.cpu().numpy())
    # gple_nlml_predict on the explicit grid points: one exponential of the summed argument where the tables multiply two
    if nx * np_ <= 257 * 257 and planes[0] is not None:
        hyper, X, b, y = planes[0]
        Xs = np.ascontiguousarray(np.stack(np.meshgrid(x, p, indexing="ij"), axis=-1).reshape(-1, 2))
        _, tol = RN.predict_plane(hyper, X, b, x, p, 1.0)
        unscaled = pred[0] if scale is None else gpu.grid_reconstruct(num_pes, model, rho, x, p, MASS, dx, dp, args)[0][0]
        assert np.all(np.abs(gpu.nlml_predict(hyper, X, y, Xs).reshape(nx, np_) - unscaled) <= 2 * tol)


def test_reconstruct_bad_arguments(gpu):
    x, p, dx, dp = grid(16, 20)
    rho = packets(2, x, p)
    X, b = np.zeros((3, 2)), np.ones(3)
    ok = [(HYPER, X, b), None, None, None]
    gpu.grid_reconstruct(2, 1, rho, x, p, MASS, dx, dp, ok)
    for kw in (dict(planes=[(HYPER * np.array([1, 1, np.inf, 1]), X, b), None, None, None]), dict(planes=[(HYPER, np.zeros((4097, 2)), np.ones(4097)), None, None, None]),
               dict(mass=-1.0), dict(model=3), dict(scale=np.array([1.0, np.nan, 1.0, 1.0])), dict(dx=np.nan)):
        with pytest.raises(_capi.GpleError):
            gpu.grid_reconstruct(2, kw.get("model", 1), rho, x, p, kw.get("mass", MASS), kw.get("dx", dx), dp, kw.get("planes", ok), kw.get("scale"))
    with pytest.raises(_capi.GpleError):
        gpu.grid_reconstruct(2, 1, rho[:, :, :1], x[:1], p, MASS, dx, dp, ok)  # one grid point along x


# ---- 9. driver --------------------------------------------------------------------------------------------------------------------------
def driver_state(n=161):
    """rho_00 a Gaussian of weight 0.7, rho_11 one of weight 0.3 elsewhere (widths 0.7 in x: both peaks far above the 1e-2 of is_small),
    rho_01 their geometric mean with the phase exp(0.5 i (x - x0))"""
    i = np.arange(n, dtype=np.float64)
    x = (-6.0 * (n - 1 - i) + 6.0 * i) / (n - 1)
    p = (12.0 * (n - 1 - i) + 28.0 * i) / (n - 1)
    sx, sp = 0.7, 0.7
    g = lambda cx, cp: np.exp(-(((x[:, None] - cx) / sx) ** 2 + ((p[None, :] - cp) / sp) ** 2) / 2.0) / (2 * math.pi * sx * sp)
    rho = np.zeros((2, 2, n, n), dtype=np.complex128)
    rho[0, 0], rho[1, 1] = 0.7 * g(-2.0, 20.0), 0.3 * g(1.0, 18.5)
    rho[0, 1] = np.sqrt(rho[0, 0].real * rho[1, 1].real) * np.exp(0.5j * (x[:, None] + 2.0))
    rho[1, 0] = np.conj(rho[0, 1])
    return x, p, rho


def check_record(gpu, rec, rho, x, p, model, n_points):
    nx, np_ = len(x), len(p)
    dx, dp = (x[-1] - x[0]) / nx, (p[-1] - p[0]) / np_
    energies = MN.Bases(x, model, 2).E
    planes_v = RN.planes_of(rho)
    assert not rec["is_small"][0] and not rec["is_small"][3]  # the two-surface branch of obey_conservation is taken
    assert np.all(np.isfinite(rec["mse_before"])) and np.all(np.isfinite(rec["mse_after"])) and np.isfinite(rec["nlml"])
    kin = p ** 2 / 2.0 / MASS
    for tag in ("before", "after"):
        pred = rec["pred_" + tag]
        for i in range(2):
            mu = pred[3 * i].astype(RN.LD)
            tol = nx * np_ * EPS
            for name, w in (("population", 1.0), ("potential", energies[:, i][:, None]), ("kinetic", kin[None, :])):
                ref, mag = (mu * w).sum() * dx * dp, np.abs(mu * w).sum() * dx * dp
                assert abs(rec[f"{name}_grid_{tag}"][i] - ref) <= tol * mag, (tag, name, i)
    # after obey_conservation the from-parameters numbers obey the two constraints: a linear solve, and b is linear in the labels
    assert not rec["singular"]
    assert abs(rec["population_gpr_after"].sum() - 1.0) <= 1e-10
    e_after = (rec["potential_gpr_after"] + rec["kinetic_gpr_after"]).sum()
    assert abs(e_after - rec["initial_energy"]) <= 1e-10 * abs(rec["initial_energy"])
    # MSE after = c^2 sum mu^2 - 2 c sum mu v + sum v^2 from the first call's sums
    s = rec["sums_before"]
    for q in range(4):
        c = rec["factors"][q]
        svv = s[q, 0] - s[q, 4] + 2 * s[q, 5]
        expect = c * c * s[q, 4] - 2 * c * s[q, 5] + svv
        tol = 4 * nx * np_ * EPS * max(1.0, c * c) * (s[q, 4] + (planes_v[q] ** 2).sum())
        print(f"driver plane {q}: factor {c:.6g} MSE before {rec['mse_before'][q]:.4g} after {rec['mse_after'][q]:.4g} (identity off by {abs(rec['mse_after'][q] - expect):.3g}, tol {tol:.3g})")
        assert abs(rec["mse_after"][q] - expect) <= tol


def test_driver_on_a_synthetic_state(gpu):
    x, p, rho = driver_state()
    model = 1
    state = reconstruct.State(gpu, 2, model, x, p, MASS)
    rec = reconstruct.reconstruct(gpu, state, rho, n_points=200, seed=20240607, maxeval=60, keep_pred=True)
    check_record(gpu, rec, rho, x, p, model, 200)
    for q in range(4):
        assert len(rec["features"][q]) == 200
    # the same state resident on the device: the same record, bit for bit
    import torch
    dev = reconstruct.reconstruct(gpu, state, torch.from_numpy(rho).cuda(), n_points=200, seed=20240607, maxeval=60, keep_pred=True)
    for key in ("hyper", "mse_before", "mse_after", "factors", "sums_before", "sums_after", "pred_after", "survey"):
        assert np.array_equal(rec[key], dev[key]), key
    # the same state 50 Trotter steps later (whatever it has become: the identities hold for every state)
    dia = gpu.mqcl_transform(2, model, x, rho, MN.ADIABATIC, MN.DIABATIC)
    dia = gpu.mqcl_evolve(2, model, x, p, dia, MASS, x[-1] - x[0], p[-1] - p[0], 0.5, 50)
    adia = gpu.mqcl_observe(2, model, x, p, dia, MASS, 1.0, 1.0)[0]
    rec2 = reconstruct.reconstruct(gpu, state, adia, n_points=200, seed=20240608, maxeval=60, keep_pred=True, start=rec["hyper"])
    assert np.all(np.isfinite(rec2["mse_after"])) and np.all(np.isfinite(rec2["hyper"]))
    if not rec2["is_small"][0] and not rec2["is_small"][3] and not rec2["singular"]:
        assert abs(rec2["population_gpr_after"].sum() - 1.0) <= 1e-10
