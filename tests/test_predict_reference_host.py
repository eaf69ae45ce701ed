"""CPU: the extended-precision row-by-row reference of the predict contraction (tests/predict_reference.py) and its derived bound, with
numpy's T = inv(chol(K)) standing in for the library's factor.  The bound must hold for an honest fp64 evaluation with room to spare and
must be violated, on every row or nearly, by the mistakes a contraction kernel can make: a k-step skipped, one element dropped."""
import numpy as np
import pytest

from tests import parity
from tests import predict_reference as PR
from tests.test_gpu_configs import THETA_C, complex_rect_kernels

M = 300
CASES = [(1000, 1e-2, 11), (700, 5e-2, 12)]
_cache = {}


def stand_in(N, sn, seed):
    """numpy's factor of the padded fp64 Gram matrix, the typed K*, the reference and an fp64 BLAS evaluation of the contraction — computed once"""
    key = (N, sn, seed)
    if key not in _cache:
        theta = [1.0, 0.7086, 0.7056, sn]
        X, _, Xs = parity.synthetic_real(N, M, seed)
        n = PR.round_up(N, PR.TILE)
        Kxx, _, _ = PR.real_kstar(theta, X, X, n)
        Kp = np.eye(n)
        Kp[:N] = Kxx.astype(np.float64)
        T = np.linalg.inv(np.linalg.cholesky(Kp))
        T = np.tril(T)
        K, a, eta = PR.real_kstar(theta, Xs, X, n)
        q_ref, bound = PR.contraction(T, K, a, eta)
        K64 = K.astype(np.float64)
        for arr in (T, K64, bound):
            arr.setflags(write=False)
        _cache[key] = dict(theta=theta, X=X, Xs=Xs, n=n, T=T, K=K, a=a, eta=eta, K64=K64, q_ref=q_ref, bound=bound)
    return _cache[key]


def blas_q(T, K64):
    Z = K64 @ T.T
    return (Z * Z).sum(axis=1)


@pytest.mark.parametrize("N,sn,seed", CASES)
def test_fp64_evaluation_keeps_the_bound_on_every_row(N, sn, seed):
    s = stand_in(N, sn, seed)
    r = PR.ratio(blas_q(s["T"], s["K64"]), s["q_ref"], s["bound"])
    print(f"N = {N}, sn = {sn}: max |q_fp64 - q_ref| / bound = {r:.2e}")
    assert r <= 1.0


@pytest.mark.parametrize("N,sn,seed", CASES)
def test_a_skipped_k_step_breaks_every_row(N, sn, seed):
    """one 16-column k-step of the last N-tile zeroed"""
    s = stand_in(N, sn, seed)
    T = s["T"].copy()
    T[s["n"] - PR.TILE:, 512:528] = 0.0
    err = np.abs(blas_q(T, s["K64"]).astype(PR.LD) - s["q_ref"]) / s["bound"]
    print(f"N = {N}: min / max |q_mutant - q_ref| / bound = {float(err.min()):.2e} / {float(err.max()):.2e}")
    assert np.all(err > 1.0)


@pytest.mark.parametrize("N,sn,seed", CASES)
def test_one_dropped_element_breaks_nearly_every_row(N, sn, seed):
    """A row can notice the loss of T(n0, k0) only through K*(row, k0): the column is that of the training point nearest the packet's centre,
    which every test point of the set sees, and the element the largest one below the diagonal in that column (an arbitrary element, T(700, 300)
    at N = 1000, is missed by the 50 rows that lie far from training point 300 — whatever the bound)"""
    s = stand_in(N, sn, seed)
    T = s["T"].copy()
    k0 = int(np.argmin((((s["X"] - [-10.0, 14.112]) / [0.7086, 0.7056]) ** 2).sum(axis=1)))
    n0 = k0 + 1 + int(np.argmax(np.abs(T[k0 + 1:, k0])))
    assert T[n0, k0] != 0.0
    T[n0, k0] = 0.0
    err = np.abs(blas_q(T, s["K64"]).astype(PR.LD) - s["q_ref"]) / s["bound"]
    print(f"N = {N}: T({n0},{k0}) dropped: {int((err > 1.0).sum())} of {M} rows beyond the bound")
    assert (err > 1.0).mean() >= 0.9


def test_mean_bound_holds_for_an_fp64_dot():
    s = stand_in(*CASES[0])
    rng = np.random.default_rng(3)
    v = np.zeros(s["n"])
    v[:1000] = rng.standard_normal(1000) * 100.0
    mu, bound = PR.mean(s["K"], s["a"], v, s["eta"])
    r = PR.ratio(s["K64"] @ v, mu, bound)
    print(f"mean: max |mu_fp64 - mu_ref| / bound = {r:.2e}")
    assert r <= 1.0


def test_lower_factor_rejects_what_no_kernel_may_read():
    s = stand_in(*CASES[1])
    T = s["T"].copy()
    T[:64, 64:128] = np.nan  # an unwritten block above the diagonal: ignored
    assert np.array_equal(PR.lower_factor(T), s["T"])
    T[3, 5] = 1e-30          # above the diagonal inside a diagonal block: read by the kernels, must be zero
    with pytest.raises(AssertionError):
        PR.lower_factor(T)


def test_typed_complex_gram_is_the_embedding_of_k_and_k_tilde():
    """The module's [Re; Im] Gram matrix on a training set: consistent with K, K~ of complex_rect_kernels (K = C_RR + C_II,
    K~ = C_RR - C_II + 2i C_RI, plus the noise on K's diagonal), symmetric, and factorised by numpy to T K T^T = I"""
    N, Np = 150, 256
    X, _, _ = parity.synthetic_real(N, 1, 21)
    G = PR.complex_gram(THETA_C, X, Np)
    n = 2 * Np
    assert np.array_equal(G, G.T)
    RR, RI, II = (G[:N, :N], G[:N, Np:Np + N], G[Np:Np + N, Np:Np + N])
    Kc, Kt = complex_rect_kernels(THETA_C, X, X)
    Kc = Kc + THETA_C[0] ** 2 * THETA_C[7] ** 2 * np.eye(N)
    scale = np.abs(Kc).max()
    assert np.abs((RR + II).astype(np.float64) - Kc).max() <= 64 * PR.U * scale
    assert np.abs((RR - II).astype(np.float64) - Kt.real).max() <= 64 * PR.U * scale
    assert np.abs((2 * RI).astype(np.float64) - Kt.imag).max() <= 64 * PR.U * scale
    pad = np.concatenate([np.arange(N, Np), np.arange(Np + N, n)])
    assert np.array_equal(G[pad], np.eye(n, dtype=PR.LD)[pad])
    G64 = G.astype(np.float64)
    T = np.tril(np.linalg.inv(np.linalg.cholesky(G64)))
    res, bound = PR.factor_residual(T, G64)
    print(f"complex embedding, n = {n}: ||T K T^T - I||_max = {res:.2e} (bound {bound:.2e})")
    assert res <= bound
    assert PR.padding_is_identity(T, N, Np)
