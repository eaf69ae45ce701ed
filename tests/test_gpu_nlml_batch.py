"""GPU: B NLML problems in one launch (gple_nlml_batch, csrc/gple_nlml_batch.hip) and the search of several planes in lock-step on it
(gple_nlml_fit_planes, reconstruct.optimize_planes).  Sizes: inside one 64-panel with padding (1, 37), exactly one panel (64), the
first trailing update with a one-row second panel (65), two and three panels with padding (130, 200), the limit (256).  Hyper-parameters are
those of test_nlml_value_gradient_and_prediction, with the cross weight c = +-0.4 for the five-parameter kernel.  eps = 2^-53."""
import ctypes as C
import functools

import numpy as np
import pytest

from gaussian_process_liouville_equation_amd import _capi, reconstruct
from tests import parity

pytestmark = pytest.mark.gpu
EPS = parity.EPS
SIZES = [1, 37, 64, 65, 130, 200, 256]
KERNELS = [None, 0.4, -0.4]  # the diagonal kernel, the cross-term kernel with c = +-0.4
BAD_ARG = 1  # GPLE_ERR_BAD_ARG


def hyper(c):
    return np.array([0.1, 1.2, 1.0 / 0.8, 1.0 / 0.7] if c is None else [0.1, 1.2, 1.0 / 0.8, c, 1.0 / 0.7])


@functools.lru_cache(maxsize=None)
def data(N):
    X, y, _ = parity.synthetic_real(N, 4, 700 + N)
    return np.ascontiguousarray(X), np.ascontiguousarray(y)


def gram(x, X):
    wd, wg, a, c, b = x if len(x) == 5 else (x[0], x[1], x[2], 0.0, x[3])
    e0, e1 = X[:, None, 0] - X[None, :, 0], X[:, None, 1] - X[None, :, 1]
    return wg ** 2 * np.exp(-0.5 * ((a * e0 + c * e1) ** 2 + (b * e1) ** 2)) + wd ** 2 * np.eye(len(X))


@functools.lru_cache(maxsize=None)
def numpy_reference(N, c):
    """(value in the form of test_nlml_at_baseline_sizes, weights, cond) from numpy, once per case"""
    X, y = data(N)
    K = gram(hyper(c), X)
    L = np.linalg.cholesky(K)
    z = np.linalg.solve(L, y)
    return 0.5 * z @ z + np.log(np.diag(L)).sum(), np.linalg.solve(K, y), np.linalg.cond(K)


@functools.lru_cache(maxsize=None)
def batch_of_all_sizes(gpu, c):
    x = hyper(c)
    return gpu.nlml_batch([x] * len(SIZES), [data(N)[0] for N in SIZES], [data(N)[1] for N in SIZES], want_grad=True, want_weights=True)


@pytest.mark.parametrize("c", KERNELS)
def test_value_gradient_and_weights(gpu, oracle, c):
    """one batch of all sizes: value against numpy's Cholesky within 50 cond eps |ref| + 1e-9 |ref|, gradient against the oracle within
    1e-7 max|grad| and against gple_nlml / gple_nlml_cross within twice that, weights against numpy.linalg.solve within 50 cond eps |b|_inf"""
    x = hyper(c)
    values, grads, weights, info = batch_of_all_sizes(gpu, c)
    assert values.shape == (len(SIZES),) and grads.shape == (len(SIZES), len(x)) and not info.any()
    for k, N in enumerate(SIZES):
        X, y = data(N)
        ref, b_ref, cond = numpy_reference(N, c)
        _, g_oracle = oracle.nlml(x, X, y)
        v_single, g_single = gpu.nlml(x, X, y)
        scale = np.abs(g_oracle).max()
        print(f"N={N} c={c}: cond {cond:.3g} value err {abs(values[k] - ref):.3g} (bound {50 * cond * EPS * abs(ref) + 1e-9 * abs(ref):.3g}) "
              f"grad - oracle {np.abs(grads[k] - g_oracle).max() / scale:.3g} grad - gple_nlml {np.abs(grads[k] - g_single).max() / scale:.3g} "
              f"weights err {np.abs(weights[k] - b_ref).max():.3g} (bound {50 * cond * EPS * np.abs(b_ref).max():.3g})")
        assert abs(values[k] - ref) <= 50 * cond * EPS * abs(ref) + 1e-9 * abs(ref)
        assert np.abs(grads[k] - g_oracle).max() <= 1e-7 * scale
        assert np.abs(grads[k] - g_single).max() <= 2e-7 * scale
        assert weights[k].shape == (N,) and np.abs(weights[k] - b_ref).max() <= 50 * cond * EPS * np.abs(b_ref).max()


def test_cross_with_c_zero_is_the_diagonal_call(gpu):
    four, five = batch_of_all_sizes(gpu, None), batch_of_all_sizes(gpu, 0.0)
    assert np.array_equal(four[0], five[0]) and np.array_equal(four[1], five[1][:, [0, 1, 2, 4]])
    assert all(np.array_equal(a, b) for a, b in zip(four[2], five[2]))


def test_a_problem_depends_on_nothing_but_itself(gpu):
    """a mixed batch of 70 problems in shuffled order: every problem's bits are those of the problem alone (B = 1); value-only, a repeat and a
    call on device arrays return the same bits"""
    import torch
    x = hyper(0.4)
    alone = {N: gpu.nlml_batch([x], [data(N)[0]], [data(N)[1]], want_weights=True) for N in SIZES}
    order = np.random.default_rng(5).permutation(np.repeat([200, 1, 65, 256, 37, 64, 130], 10))
    Xs, ys = [data(N)[0] for N in order], [data(N)[1] for N in order]
    values, grads, weights, info = gpu.nlml_batch([x] * len(order), Xs, ys, want_weights=True)
    for k, N in enumerate(order):
        assert values[k] == alone[N][0][0] and np.array_equal(grads[k], alone[N][1][0]) and np.array_equal(weights[k], alone[N][2][0]), (k, N)
    assert not info.any() and np.all(np.isfinite(values)) and np.all(np.isfinite(grads))
    only, none, _, _ = gpu.nlml_batch([x] * len(order), Xs, ys, want_grad=False)
    assert none is None and np.array_equal(only, values)
    again = gpu.nlml_batch([x] * len(order), Xs, ys, want_weights=True)
    assert np.array_equal(again[0], values) and np.array_equal(again[1], grads)
    dv, dg, dw, di = gpu.nlml_batch([x] * len(order), [torch.from_numpy(X).cuda() for X in Xs], [torch.from_numpy(y).cuda() for y in ys], want_weights=True)
    gpu.synchronize()
    assert dv.is_cuda and np.array_equal(dv.cpu().numpy(), values) and np.array_equal(dg.cpu().numpy(), grads) and not di.cpu().numpy().any()
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(dw, weights))


def test_non_positive_pivot_is_nan_for_that_problem_only(gpu):
    """two identical points with w_d = 0, w_g = 1: the second pivot is 1 - 1 = 0.  NaN and the column in info for that problem; its neighbours
    in the launch return the bits they return without it"""
    good = [(hyper(None), *data(37)), (hyper(None), *data(65))]
    twin = (np.array([0.0, 1.0, 1.0, 1.0]), np.array([[0.5, 14.0], [0.5, 14.0]]), np.array([1.0, 2.0]))
    with_it = gpu.nlml_batch(*zip(good[0], twin, good[1]), want_weights=True)
    without = gpu.nlml_batch(*zip(*good), want_weights=True)
    assert np.isnan(with_it[0][1]) and np.all(np.isnan(with_it[1][1])) and np.all(np.isnan(with_it[2][1])) and with_it[3].tolist() == [0, 2, 0]
    for k_with, k_without in ((0, 0), (2, 1)):
        for part in range(3):
            assert np.array_equal(with_it[part][k_with], without[part][k_without])
    assert np.all(np.isfinite(without[0])) and np.all(np.isfinite(without[1]))


def test_bad_arguments(gpu):
    x, (X, y) = hyper(None), data(37)
    with pytest.raises(_capi.GpleError):
        gpu.nlml_batch([x], [X[:0]], [y[:0]])
    big = np.ascontiguousarray(np.tile(X, (7, 1))[:257])
    with pytest.raises(_capi.GpleError):
        gpu.nlml_batch([x], [big], [np.zeros(257)])
    probs = (_capi.NlmlProblem * 1)()
    probs[0].x = (C.c_double * 5)(*x, 0.0)
    probs[0].X, probs[0].y, probs[0].N = _capi._ptr(X), _capi._ptr(y), len(X)
    value, f = C.c_double(), gpu.lib.gple_nlml_batch
    assert f(gpu.ctx, probs, 1, 0, 0, C.byref(value), None, None, None) == 0 and np.isfinite(value.value)
    assert f(gpu.ctx, probs, 0, 0, 0, C.byref(value), None, None, None) == BAD_ARG
    assert f(gpu.ctx, None, 1, 0, 0, C.byref(value), None, None, None) == BAD_ARG
    assert f(gpu.ctx, probs, 1, 0, 0, None, None, None, None) == BAD_ARG
    probs[0].y = None
    assert f(gpu.ctx, probs, 1, 0, 0, C.byref(value), None, None, None) == BAD_ARG
    plane = (_capi.NlmlFitPlane * 1)()
    out, ne = np.empty(6), C.c_int()
    assert gpu.lib.gple_nlml_fit_planes(gpu.ctx, plane, 1, 0, None, _capi._ptr(out), _capi._ptr(out[5:]), C.byref(ne), None) == BAD_ARG  # null X, N = 0
    assert gpu.lib.gple_nlml_fit_planes(gpu.ctx, plane, 0, 0, None, _capi._ptr(out), _capi._ptr(out[5:]), C.byref(ne), None) == BAD_ARG


class BatchEvaluated:
    """an Api whose nlml is a one-problem gple_nlml_batch: reconstruct.optimize on it is the library's search on the batched evaluator"""

    def __init__(self, gpu):
        self.gpu, self.lib = gpu, gpu.lib

    def nlml(self, x, X, y, want_grad=True):
        v, g, _, _ = self.gpu.nlml_batch([x], [X], [y], want_grad=want_grad)
        return float(v[0]), (g[0] if want_grad else None)


@pytest.mark.parametrize("c", [None, 0.4])
def test_fit_planes_is_the_same_search_plane_by_plane(gpu, c):
    """P = 4 planes in lock-step (every Nelder-Mead step's four candidates in one request): each plane's (x, f, n_eval) is bit for bit that of
    the same entry on the plane alone, and that of reconstruct.optimize on a one-problem batched evaluator"""
    sizes = [37, 64, 65, 200]
    big = reconstruct.DBL_MAX
    start = hyper(c)
    lower, upper = np.array([1e-3, 1e-2, 0.05, 0.05]), np.array([1.0, 10.0, big, big])
    if c is not None:
        lower, upper = np.insert(lower, 3, -big), np.insert(upper, 3, big)
    options = reconstruct._options(300)
    planes = [(*data(N), start, lower, upper) for N in sizes]
    xs, fs, ns, ws = gpu.nlml_fit_planes(planes, cross=c is not None, options=options, want_weights=True)
    assert xs.shape == (4, len(start)) and np.all(xs >= lower) and np.all(xs <= upper) and np.all(ns > 0)
    shim = BatchEvaluated(gpu)
    for k, N in enumerate(sizes):
        x1, f1, n1, w1 = gpu.nlml_fit_planes(planes[k:k + 1], cross=c is not None, options=options, want_weights=True)
        assert np.array_equal(x1[0], xs[k]) and f1[0] == fs[k] and n1[0] == ns[k] and np.array_equal(w1[0], ws[k]), N
        xo, fo, no = reconstruct.optimize(shim, *data(N), start, lower, upper, maxeval=300)
        assert np.array_equal(xo, xs[k]) and fo == fs[k] and no == ns[k], (N, xo, xs[k], fo, fs[k], no, ns[k])
        at_result, at_start = gpu.nlml(xs[k], *data(N), want_grad=False)[0], gpu.nlml(start, *data(N), want_grad=False)[0]
        print(f"N={N} c={c}: NLML {at_start:.6g} -> {at_result:.6g} at {xs[k]} after {ns[k]} evaluations")
        assert at_result <= at_start
        # the weights handed over are those of the result
        b = gpu.nlml_batch([xs[k]], [data(N)[0]], [data(N)[1]], want_grad=False, want_weights=True)[2][0]
        assert np.array_equal(b, ws[k])


def test_driver_with_the_batched_fit(gpu):
    """reconstruct(..., fit="batched") on the synthetic two-level state of tests/test_gpu_recon.py: the record of the serial fit in keys and
    shapes, the two constraints to 1e-10 and the MSE identity from the first call's sums (check_record)"""
    from tests.test_gpu_recon import MASS, check_record, driver_state
    x, p, rho = driver_state()
    model = 1
    state = reconstruct.State(gpu, 2, model, x, p, MASS)
    rec = reconstruct.reconstruct(gpu, state, rho, n_points=200, seed=20240607, maxeval=60, keep_pred=True, fit="batched")
    check_record(gpu, rec, rho, x, p, model, 200)
    serial = reconstruct.reconstruct(gpu, state, rho, n_points=200, seed=20240607, maxeval=60, keep_pred=True)
    assert set(rec) == set(serial)
    for key in set(rec) - {"seconds", "cells", "features", "labels", "draws"}:
        assert np.shape(rec[key]) == np.shape(serial[key]), key
    assert all(np.array_equal(a, b) for a, b in zip(rec["features"], serial["features"]))
    print(f"NLML serial {serial['nlml']:.6g} batched {rec['nlml']:.6g}; optimize {1e3 * serial['seconds']['optimize']:.1f} ms -> {1e3 * rec['seconds']['optimize']:.1f} ms")
