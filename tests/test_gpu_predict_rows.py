"""GPU (MI355X): every path of the predict contraction, every row, against the extended-precision evaluation of the same operation on the
same fp64 operands (tests/predict_reference.py) — the factor T comes from gple_debug_fit_factor, the weights from the getters, K* from the
public parameters.  The bound is derived there, per row, from the number formats; nothing here is tuned.  Every case asserts which kernel ran.

Measured max |error| / bound per case and what four deliberate mistakes in the kernels did to these tests: DESIGN.md §5."""
import ctypes as C
import os

import numpy as np
import pytest

from gaussian_process_liouville_equation_amd import _capi as c
from tests import parity
from tests import predict_reference as PR
from tests.test_gpu_configs import THETA_C, THETA_R

pytestmark = pytest.mark.gpu

CENTRE, SCALE = np.array([-10.0, 14.112]), np.array([0.7086, 0.7056])  # the packet; the length scales of THETA_R and of every block of THETA_C
FUSED, R3, GEMM = "predict_fused256_kernel", "rownorm3_kernel", "gemm_f64 (Z = T K*^T) + colsumsq_kernel"
FULL = c.PREDICT_FULL


def rownorm(pipe, blocking, queue):
    return f"rownorm{'p' if pipe else '2'}_kernel<{blocking},{'true' if queue else 'false'}>"


def dead_points(X, count, rng):
    """points whose nearest training point is 8 to 40 length scales away: nothing the pruned predict contracts"""
    out = np.empty((0, 2))
    reach = np.sqrt((((X - CENTRE) / SCALE) ** 2).sum(axis=1)).max()
    while len(out) < count:
        phi, r = rng.uniform(0, 2 * np.pi, 4 * count), reach + rng.uniform(4.0, 40.0, 4 * count)
        cand = CENTRE + SCALE * np.stack([r * np.cos(phi), r * np.sin(phi)], axis=1)
        dmin = np.sqrt(((((cand[:, None, :] - X[None, :, :]) / SCALE) ** 2).sum(axis=2)).min(axis=1))
        out = np.concatenate([out, cand[(dmin >= 8.0) & (dmin <= 40.0)]])
    return out[:count]


def query_points(X, M, seed):
    """Training points plus N(0, 0.3^2) noise (K* entries of order one), three rows exactly on training points (the delta term) and dead rows.
    From 128 rows on: 128-row block 0 mixes live and dead rows (every fourth is dead), block 1 is entirely dead, the blocks after it — the
    ragged last one — mix again.  Below 128 rows: one mixed block."""
    rng = np.random.default_rng(seed)
    pts = X[rng.integers(0, len(X), M)] + rng.normal(0.0, 0.3, (M, 2))
    rows = np.arange(M)
    dead = (rows % 4 == 3) | ((rows >= 128) & (rows < 256))
    exact = [r for r in (0, 1, M - 1 if M <= 128 or M > 256 else 2) if r < M]
    dead[exact] = False
    pts[dead] = dead_points(X, int(dead.sum()), rng)
    pts[exact] = X[rng.integers(0, len(X), len(exact))]
    return np.ascontiguousarray(pts), dead


class Knobs:
    """gple_debug_predict_knobs for the length of a `with`: 0 / 1 set a knob, 2 = the default"""

    def __init__(self, gpu):
        self.gpu, self.fn = gpu, gpu.lib.gple_debug_predict_knobs
        self.fn.argtypes, self.fn.restype = [C.c_void_p, C.c_int, C.c_int], C.c_int

    def set(self, pipe=2, fused=2):
        assert self.fn(self.gpu.ctx, pipe, fused) == 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.set(2, 2)


def check_factor(fit, Kpad):
    """the getter, once per fit: T K T^T = I on the padded system, the identity on the padding -> T[n, k]"""
    T, n_split, N = fit.debug_factor()
    n = T.shape[0]
    assert N == fit.N and n_split == PR.round_up(N, 256) and n == (2 if fit.kind == "complex" else 1) * n_split and Kpad.shape == (n, n)
    res, bound = PR.factor_residual(T, Kpad)
    print(f"  {fit.kind} N = {N}, n_total = {n}: ||T K T^T - I||_max = {res:.2e} (bound {bound:.2e})")
    assert res <= bound
    assert PR.padding_is_identity(T, N, n_split)
    return T, n_split


def real_fit_and_factor(gpu, N, theta, seed):
    X, y, _ = parity.synthetic_real(N, 1, seed)
    fit = gpu.real_fit(theta, X, y, 0)
    assert fit.scalars["info"] == 0
    n = PR.round_up(N, 256)
    Kpad = np.eye(n)
    Kpad[:N, :N] = fit.get(c.R_KERNEL)
    T, _ = check_factor(fit, Kpad)
    return X, fit, T, fit.get(c.R_INVLBL)


def complex_fit_and_factor(gpu, N, seed):
    X, yr, _ = parity.synthetic_real(N, 1, seed)
    y = 0.5 * yr * np.exp(0.5j * (X[:, 0] - CENTRE[0]))
    fit = gpu.complex_fit(THETA_C, X, y, 0)
    assert fit.scalars["info"] == 0
    Np = PR.round_up(N, 256)
    T, n_split = check_factor(fit, PR.complex_gram(THETA_C, X, Np).astype(np.float64))
    return X, fit, T, fit.get(c.C_INVLBL), n_split


def compare(label, p, ref, kernel, expected, dead, shown=None):
    """all rows of the call, none sampled: max |error| / bound of the variance and of the mean, printed and held to 1.  (The variance of a dead
    row is k** itself and its bound the 4 u k** of the subtraction, and its mean hangs on one or two K* entries with an exponent argument of
    several hundred: the figures of the live rows alone are printed beside those of all rows.)"""
    assert kernel == expected, (label, kernel, expected)
    live = ~dead[:len(p["variance"])]
    parts = [(p["prediction"].real, ref["mean"][0], ref["mean_bound"][0]), (p["prediction"].imag, ref["mean"][1], ref["mean_bound"][1])] \
        if isinstance(ref["mean"], tuple) else [(p["prediction"], ref["mean"], ref["mean_bound"])]
    rv, rl = PR.ratio(p["variance"], ref["var"], ref["var_bound"]), PR.ratio(p["variance"][live], ref["var"][live], ref["var_bound"][live])
    rm, rml = max(PR.ratio(*t) for t in parts), max(PR.ratio(*(x[live] for x in t)) for t in parts)
    print(f"  {label:58s} {shown or kernel:42s} variance {rv:.2e} (live rows {rl:.2e})  mean {rm:.2e} (live rows {rml:.2e})   max |error| / bound over {len(live)} rows")
    assert np.all(np.isfinite(p["variance"])) and rv <= 1.0 and rm <= 1.0, (label, rv, rm)


def run_real(gpu, monkeypatch, N, Ms, configs, theta=THETA_R, seed=0):
    """one fit, one reference per M, one predict per (small_m, flags, pipe, fused, expected kernel)"""
    X, fit, T, v = real_fit_and_factor(gpu, N, theta, 100 + N + seed)
    with Knobs(gpu) as knobs:
        for M in Ms:
            Xs, dead = query_points(X, M, 200 + N + M)
            ref = PR.real_reference(theta, T, v, X, Xs)
            for small_m, flags, pipe, fused, expected in configs:
                if small_m is None:
                    monkeypatch.delenv("GPLE_PREDICT_SMALL_M", raising=False)
                else:
                    monkeypatch.setenv("GPLE_PREDICT_SMALL_M", small_m)
                knobs.set(pipe, fused)
                p = gpu.real_predict(fit, Xs, flags=flags)
                compare(f"real N = {N}, sn = {theta[3]:g}, M = {M}, {'full' if flags & FULL else 'pruned'}, pipe {pipe}, fused {fused}, small_m {small_m}",
                        p, ref, gpu.last_contraction_kernel(), expected, dead)
    fit.release()


def streaming(blocking):
    """full and pruned, both contraction kernels: (small_m, flags, pipe, fused, kernel)"""
    return [("0", FULL, 1, 2, rownorm(1, blocking, False)), ("0", 0, 1, 2, rownorm(1, blocking, True)),
            ("0", FULL, 0, 2, rownorm(0, blocking, False)), ("0", 0, 0, 2, rownorm(0, blocking, True))]


def test_factor_getter_sizes_and_errors(gpu):
    """the sizes come back without a buffer; a buffer one double short, both handles and no handle are errors that copy nothing"""
    X, y, _ = parity.synthetic_real(300, 1, 7)
    fit = gpu.real_fit(THETA_R, X, y, 0)
    fn = gpu.lib.gple_debug_fit_factor
    nt, ns, N = C.c_int(), C.c_int(), C.c_int()
    assert fn(fit.handle, None, None, 0, C.byref(nt), C.byref(ns), C.byref(N)) == 0 and (nt.value, ns.value, N.value) == (512, 512, 300)
    buf = np.full(512 * 512, 7.0)
    ptr = buf.ctypes.data_as(C.POINTER(C.c_double))
    assert fn(fit.handle, None, ptr, buf.size - 1, None, None, None) == 1  # GPLE_ERR_BAD_ARG
    assert fn(fit.handle, fit.handle, ptr, buf.size, None, None, None) == 1
    assert fn(None, None, ptr, buf.size, None, None, None) == 1
    assert np.all(buf == 7.0)
    assert fn(fit.handle, None, ptr, buf.size, None, None, None) == 0
    T, n_split, n = fit.debug_factor()
    assert np.array_equal(buf.reshape(512, 512).T, T, equal_nan=True) and (n_split, n) == (512, 300)
    fit.release()


# ---- real fits --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [37, 255, 256])
def test_one_tile_real_fit_in_the_fused_kernel(gpu, monkeypatch, N):
    """n_total = 256, M = 65 and 200: predict_fused256_kernel by the knob and by default, pruned request included"""
    run_real(gpu, monkeypatch, N, [65, 200], [(None, FULL, 2, 1, FUSED), (None, FULL, 2, 2, FUSED), (None, 0, 2, 2, FUSED)])


def test_one_tile_real_fit_in_separate_kernels(gpu, monkeypatch):
    """the same size with the fused kernel switched off: rownorm3_kernel (full), the work-queue kernel on one N-tile (pruned)"""
    run_real(gpu, monkeypatch, 255, [200], [("0", FULL, 2, 0, R3), ("0", 0, 2, 0, rownorm(1, "2,8", True))])


@pytest.mark.parametrize("N", [257, 500])
def test_two_tiles_short_factor_kernel(gpu, monkeypatch, N):
    run_real(gpu, monkeypatch, N, [129, 300], [("0", FULL, 2, 2, R3)])


def test_two_tiles_pruned_2x8_kernels(gpu, monkeypatch):
    run_real(gpu, monkeypatch, 300, [300], [("0", 0, 1, 2, rownorm(1, "2,8", True)), ("0", 0, 0, 2, rownorm(0, "2,8", True))])


@pytest.mark.parametrize("N", [513, 768, 1000, 1025])
def test_4x4_kernels_full_and_pruned(gpu, monkeypatch, N):
    """three N-tiles (one group), four (split 2), five (split 2: an odd tile count with groups); M = 300"""
    run_real(gpu, monkeypatch, N, [300], streaming("4,4"))


def test_4x4_kernels_with_more_noise(gpu, monkeypatch):
    run_real(gpu, monkeypatch, 1000, [300], streaming("4,4")[:2], theta=[1.0, 0.7086, 0.7056, 5e-2], seed=1)


def test_nine_tiles_split_4(gpu, monkeypatch):
    run_real(gpu, monkeypatch, 2100, [200], streaming("4,4")[:2])


def test_sixteen_tiles_split_8(gpu, monkeypatch):
    run_real(gpu, monkeypatch, 4096, [130], streaming("4,4")[:1])


@pytest.mark.parametrize("N", [513, 1025])
def test_gemm_path_real(gpu, monkeypatch, N):
    run_real(gpu, monkeypatch, N, [17, 300], [("1", FULL, 2, 2, GEMM), ("1", 0, 2, 2, GEMM)])


# ---- complex fits: n_total = 2 Np, two typed rows per point, the typed split at a row-block boundary ---------------------------------------------
@pytest.mark.parametrize("N,full_kernel,queue_kernel", [(100, R3, rownorm(1, "2,8", True)), (300, rownorm(1, "4,4", False), rownorm(1, "4,4", True)),
                                                       (520, rownorm(1, "4,4", False), rownorm(1, "4,4", True))])
def test_complex_fits_streaming_and_gemm(gpu, monkeypatch, N, full_kernel, queue_kernel):
    X, fit, T, v, n_split = complex_fit_and_factor(gpu, N, 300 + N)
    for M in (9, 130):
        Xs, dead = query_points(X, M, 400 + N + M)
        ref = PR.complex_reference(THETA_C, T, v, X, Xs, n_split)
        for small_m, flags, expected in (("0", FULL, full_kernel), ("0", 0, queue_kernel), ("1", FULL, GEMM)):
            monkeypatch.setenv("GPLE_PREDICT_SMALL_M", small_m)
            p = gpu.complex_predict(fit, Xs, flags=flags)
            compare(f"complex N = {N}, M = {M}, {'full' if flags & FULL else 'pruned'}, small_m {small_m}", p, ref, gpu.last_contraction_kernel(), expected, dead)
    fit.release()


# ---- the few-points path ---------------------------------------------------------------------------------------------------------------------
SENTINEL = rownorm(1, "2,8", True)


def few_sentinel(gpu, monkeypatch):
    """predict_few_kernel leaves the context's contraction-kernel name alone: a predict that is known to set it goes first, and a few-points
    predict after which the name still stands has launched no other contraction.  The name is one that no predict of 16 typed rows or fewer can
    record with the default knobs and environment, whatever the size of the fit (those go to the fused kernel on one N-tile and to the GEMM path
    above): the work-queue kernel of a pruned two-tile predict with the few-rows path forced off."""
    assert os.environ.get("GPLE_PREDICT_FEW") is None
    X, y, Xs = parity.synthetic_real(300, 20, 5)
    f = gpu.real_fit(THETA_R, X, y, 0)
    monkeypatch.setenv("GPLE_PREDICT_SMALL_M", "0")
    gpu.real_predict(f, Xs)
    monkeypatch.delenv("GPLE_PREDICT_SMALL_M")
    f.release()
    assert gpu.last_contraction_kernel() == SENTINEL


def device_predict(gpu, fit, Xs):
    import torch

    M = len(Xs)
    dXs = torch.tensor(Xs, device="cuda")
    out = torch.full((3, M), float("nan"), dtype=torch.float64, device="cuda")
    dp = lambda t: C.cast(t.data_ptr(), C.POINTER(C.c_double))
    torch.cuda.synchronize()
    assert gpu.lib.gple_real_predict(gpu.ctx, fit.handle, dp(dXs), M, c.IO_DEVICE, None, dp(out[0]), dp(out[1]), dp(out[2]), None) == 0
    gpu.synchronize()
    o = out.cpu().numpy()
    return dict(prediction=o[0], variance=o[1], cutoff=o[2])


@pytest.mark.parametrize("N", [200, 600, 1100])
def test_few_points_real(gpu, monkeypatch, N):
    """n_total = 256, 768, 1280; M = 1, 2, 16 through host pointers (the pinned block), M = 2 through device pointers as well"""
    monkeypatch.delenv("GPLE_PREDICT_SMALL_M", raising=False)
    X, fit, T, v = real_fit_and_factor(gpu, N, THETA_R, 500 + N)
    Xs, dead = query_points(X, 16, 600 + N)
    ref = PR.real_reference(THETA_R, T, v, X, Xs)
    few_sentinel(gpu, monkeypatch)
    for M, device in ((1, False), (2, False), (16, False), (2, True)):
        p = device_predict(gpu, fit, Xs[:M]) if device else gpu.real_predict(fit, Xs[:M])
        sub = {k: a[:M] for k, a in ref.items()}
        compare(f"few points, real N = {N}, M = {M}, {'device' if device else 'host'} pointers", p, sub, gpu.last_contraction_kernel(), SENTINEL, dead, shown="predict_few_kernel")
    fit.release()


@pytest.mark.parametrize("N", [100, 300, 520])
def test_few_points_complex(gpu, monkeypatch, N):
    """n_total = 512, 1024, 1536 (2 Np: the sizes a complex fit can have); M = 1 and 8, i.e. 2 and 16 typed rows"""
    monkeypatch.delenv("GPLE_PREDICT_SMALL_M", raising=False)
    X, fit, T, v, n_split = complex_fit_and_factor(gpu, N, 700 + N)
    Xs, dead = query_points(X, 8, 800 + N)
    ref = PR.complex_reference(THETA_C, T, v, X, Xs, n_split)
    few_sentinel(gpu, monkeypatch)
    for M in (1, 8):
        p = gpu.complex_predict(fit, Xs[:M])
        sub = dict(mean=tuple(a[:M] for a in ref["mean"]), mean_bound=tuple(a[:M] for a in ref["mean_bound"]), var=ref["var"][:M], var_bound=ref["var_bound"][:M])
        compare(f"few points, complex N = {N}, M = {M}", p, sub, gpu.last_contraction_kernel(), SENTINEL, dead, shown="predict_few_kernel")
    fit.release()


# ---- the cut-off ---------------------------------------------------------------------------------------------------------------------------------
def ray(M):
    """outwards from the packet's centre, 2 to 4 length scales away: the mean falls from far above the standard deviation to far below it while
    the variance rises to k**, so the rows pass through all three branches of the cut-off"""
    r = np.linspace(2.0, 4.0, M)
    return np.ascontiguousarray(CENTRE + SCALE * np.stack([r, r], axis=1) / np.sqrt(2.0))


def check_cutoff(p, s, cplx, roundings):
    m, var = p["prediction"], p["variance"]
    if cplx:
        sq, ab = m.real * m.real + m.imag * m.imag, np.hypot(m.real, m.imag)
    else:
        sq, ab = m * m, np.abs(m)
    cf = PR.cutoff(sq, ab, var)
    counts = (int((cf == 1.0).sum()), int(((cf > 0.0) & (cf < 1.0)).sum()), int((cf == 0.0).sum()))
    assert min(counts) >= 3, counts
    want = (m.real * cf / s + 1j * (m.imag * cf / s)) if cplx else m * cf / s
    err = np.abs(p["cutoff"] - want)
    tol = roundings * PR.U * ab / s
    worst = float((err / np.maximum(tol, 1e-300)).max())
    print(f"  cut-off, {'complex' if cplx else 'real'}: rows with factor 1 / between / 0 = {counts}, max |error| / tolerance = {worst:.2e}")
    assert np.all(err <= tol), worst


def test_cutoff_of_both_finish_kernels_and_the_fused_epilogue(gpu, monkeypatch):
    """`cutoff` recomputed in fp64 numpy from the device's own mean and variance with the operation order of cutoff_value (gple_kernels.h) and
    of predict_finish_real_kernel / predict_finish_complex_kernel / the epilogue of predict_fused256_kernel: the same inputs, so the same
    branches (and the cubic meets both neighbours with slope zero: a row at a threshold moves by nothing either way).
    Tolerance, in units of u |mean| / rescale — the roundings of that code, each weighted with what it does to the result.  The factor is
    f(a) = (5 - 2a)(a - 1)^2 on 1 < a < 2, f <= 1 and a |f'(a)| = 6 a (a - 1)(2 - a) <= 2.4.  Real: two roundings reach a (the square root, the
    quotient; |m| is exact): 2 x 2.4; the cubic has six (6 - 2a, - 1, a - 1 in each of the two factors, the square, the product): 6; m cf and / s: 2
    — 13 u.  Complex: hypot is within one ulp, two more roundings into a: 2 x 2.4 — 18 u.  An IEEE-exact device evaluation (what the code compiles
    to: no operation here can be contracted except re re + im im, which only feeds the branches) gives 0; hypot may differ by an ulp."""
    monkeypatch.delenv("GPLE_PREDICT_SMALL_M", raising=False)
    Xs = ray(256)
    for N, expected in ((300, GEMM), (200, FUSED)):  # (two row blocks on two N-tiles: the few-rows path by default)
        X, y, _ = parity.synthetic_real(N, 1, 900 + N)
        fit = gpu.real_fit(THETA_R, X, y, 0)
        p = gpu.real_predict(fit, Xs)
        assert gpu.last_contraction_kernel() == expected
        check_cutoff(p, fit.scalars["rescale_factor"], False, 13)
        fit.release()
    X, yr, _ = parity.synthetic_real(100, 1, 903)
    fit = gpu.complex_fit(THETA_C, X, 0.5 * yr * np.exp(0.5j * (X[:, 0] - CENTRE[0])), 0)
    p = gpu.complex_predict(fit, Xs)
    assert gpu.last_contraction_kernel() == GEMM
    check_cutoff(p, fit.scalars["rescale_factor"], True, 18)
    fit.release()
