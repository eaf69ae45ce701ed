"""Extended-precision reference of the predict contraction, row by row, with a derived error bound (numpy only, no GPU).

What the library computes for a test row with typed kernel row k (gple_predict.hip):
    q   = sum_n z_n^2,  z = T k        T = chol(K)^-1, lower triangular, padded to n_total (a multiple of 256) with the identity
    var = self - q                      (complex GP, the real system of [Re; Im]: self - (q_re + q_im), two typed rows per point)
    mu  = k . v                         v = K^-1 ys
The reference evaluates the same operations on the same fp64 operands — T as gple_debug_fit_factor hands it out, v from the getters, K* from
the public parameters — in np.longdouble (x87: 64-bit mantissa).  Its own rounding is 2^-11 of every term below and is ignored.

The bound, per row (u = 2^-53, gamma_m = m u / (1 - m u)):
    g_k = 4 + 6 a_k                          proven relative error of a Gram entry in units of u, a_k its exponent argument
                                             (parity.check_gram_ulp(proven=True))
    A_n = sum_k |T(n,k)| |k_k|,  G_n = sum_k |T(n,k)| |k_k| g_k
    m   = 2 n_total + 8                      products rounded separately or fused, any summation order, the eight virtual-group partial sums
    e_n = u G_n + gamma_m (A_n + u G_n)      |z^_n - z_n|
    |q^ - q_ref|     <= sum_n (2 |z_n| e_n + e_n^2) + gamma_m sum_n (|z_n| + e_n)^2
    |var^ - var_ref| <= that (both typed rows for complex) + 4 u self
    |mu^ - mu_ref|   <= u sum_k g_k |k_k| |v_k| + gamma_{n_total + 64} sum_k |k_k| |v_k|      (64 = GEN_KSPLIT_MAX partial sums)
A and G are plain fp64 matrix products.

Underflow.  fl(x op y) = (x op y)(1 + d), |d| <= u, is the precision of fp64 in its normal range only; a result below 2^-1022 carries an
absolute error of up to 2^-1074 instead.  A test row 38 and more length scales from every training point has K* entries there (the reference's
long double does not underflow), so every bound carries the absolute counterpart of its relative terms, written `eta` below: an entry
k = amp (exp(-a) + n2 delta) is off by at most (amp + 1) 2^-1074 more (the exponential, the product), every product T(n,k) k_k, z_n z_n and
k_k v_k by 2^-1074 more; sums that underflow are exact.  These terms are of the order 1e-320 and decide nothing outside that range.
"""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 2.0 ** -60, "np.longdouble is no extended type on this platform: the row-by-row reference needs one"

U = 2.0 ** -53
TINY = 2.0 ** -1074      # spacing of fp64 below its normal range
TILE = 256               # N-tile of the contraction kernels (BN)
BLOCK = 64               # block of the factorisation: the blocks of T above the diagonal are never written
GEN_KSPLIT_MAX = 64      # partial sums of the mean (gple_predict.hip)


def gamma(m):
    return m * U / (1.0 - m * U)


def round_up(n, m):
    return (n + m - 1) // m * m


def lower_factor(T):
    """The factor as the kernels use it: T (n, n) float64 with T[n, k], n a multiple of 256.  The strict upper triangle INSIDE the diagonal
    64-blocks must be exactly zero and the lower triangle finite (asserted); the 64-blocks above the diagonal are unwritten memory (NaN in a
    poisoned test session) and come back as zeros."""
    n = T.shape[0]
    assert T.shape == (n, n) and n % TILE == 0
    for b in range(0, n, BLOCK):
        d = T[b:b + BLOCK, b:b + BLOCK]
        assert np.all(np.triu(d, 1) == 0.0), f"diagonal block at {b}: entries above the diagonal"
    L = np.tril(T)
    assert np.all(np.isfinite(L))
    return L


def _exponent(Xs, X, l0, l1):
    d0 = (Xs[:, None, 0].astype(LD) - X[None, :, 0].astype(LD)) / LD(l0)
    d1 = (Xs[:, None, 1].astype(LD) - X[None, :, 1].astype(LD)) / LD(l1)
    return (d0 * d0 + d1 * d1) / LD(2)


def _coincide(Xs, X):
    return ((Xs[:, None, 0] == X[None, :, 0]) & (Xs[:, None, 1] == X[None, :, 1])).astype(LD)


def real_self(theta):
    sf, sn = LD(theta[0]), LD(theta[3])
    return sf * sf * (1 + sn * sn)


def real_kstar(theta, Xs, X, n_total):
    """K* = sf^2 (exp(-a) + sn^2 delta), a = (d0^2 + d1^2) / 2, delta exact coincidence; padded columns 0.
    -> (K (M, n_total) long double, a (M, n_total) float64, eta (n_total,) float64: the absolute error of an entry under underflow)"""
    M, N = len(Xs), len(X)
    sf, sn = LD(theta[0]), LD(theta[3])
    a = _exponent(Xs, X, theta[1], theta[2])
    K = np.zeros((M, n_total), dtype=LD)
    K[:, :N] = sf * sf * (np.exp(-a) + sn * sn * _coincide(Xs, X))
    af = np.zeros((M, n_total))
    af[:, :N] = a
    return K, af, np.full(n_total, (float(sf * sf) + 1.0) * TINY)


def complex_blocks(theta, A, B):
    """s^2 K_R, s^2 K_I, s^2 K_C between two point sets (no noise) and their exponent arguments, in long double
    (complex_kernel.cpp:134-164; tests/test_gpu_configs.py::complex_rect_kernels is K = s^2 (K_R + K_I), K~ = s^2 (K_R - K_I + 2i K_C))"""
    s, sR, lR0, lR1, sI, lI0, lI1, _ = (LD(t) for t in theta)
    ss0, ss1 = lR0 * lR0 + lI0 * lI0, lR1 * lR1 + lI1 * lI1
    sC2 = sR * sI * (2 * lR0 * lI0 / ss0) * (2 * lR1 * lI1 / ss1)
    aR, aI, aC = _exponent(A, B, lR0, lR1), _exponent(A, B, lI0, lI1), _exponent(A, B, np.sqrt(ss0 / 2), np.sqrt(ss1 / 2))
    amps = (s * s * sR * sR, s * s * sI * sI, s * s * sC2)
    return (amps[0] * np.exp(-aR), amps[1] * np.exp(-aI), amps[2] * np.exp(-aC)), (aR, aI, aC), amps


def complex_self(theta):
    s, sR, sI, sn = LD(theta[0]), LD(theta[1]), LD(theta[4]), LD(theta[7])
    return s * s * (sR * sR + sI * sI + sn * sn)


def complex_kstar(theta, Xs, X, n_split):
    """The two typed rows of every point in the [Re; Im] embedding (split at n_split, n_total = 2 n_split): a Re-type row is
    [s^2 K_R, s^2 K_C], an Im-type row [s^2 K_C, s^2 K_I]; the noise s^2 sn^2 / 2 sits on coincident points of equal type
    (gple_capi.hip, the prune_thr comment); padded columns 0.
    -> ((K_re, a_re, eta_re), (K_im, a_im, eta_im)), each as real_kstar returns"""
    M, N = len(Xs), len(X)
    (KR, KI, KC), (aR, aI, aC), amps = complex_blocks(theta, Xs, X)
    noise = LD(theta[0]) ** 2 * LD(theta[7]) ** 2 / 2 * _coincide(Xs, X)
    out = []
    for first, second, a1, a2, amp1, amp2 in ((KR + noise, KC, aR, aC, amps[0], amps[2]), (KC, KI + noise, aC, aI, amps[2], amps[1])):
        K, a, eta = np.zeros((M, 2 * n_split), dtype=LD), np.zeros((M, 2 * n_split)), np.zeros(2 * n_split)
        K[:, :N], K[:, n_split:n_split + N] = first, second
        a[:, :N], a[:, n_split:n_split + N] = a1, a2
        eta[:n_split], eta[n_split:] = (float(amp1) + 1.0) * TINY, (float(amp2) + 1.0) * TINY
        out.append((K, a, eta))
    return tuple(out)


def complex_gram(theta, X, n_split):
    """The padded Gram matrix of the [Re; Im] embedding on the training set itself (identity on the padding), long double"""
    N = len(X)
    (kre, _, _), (kim, _, _) = complex_kstar(theta, X, X, n_split)
    K = np.eye(2 * n_split, dtype=LD)
    K[:N] = kre
    K[n_split:n_split + N] = kim
    return K


def contraction(T, K, a, eta=0.0):
    """q_ref(row) = sum_n z_n^2, z = T k in long double, and the bound on |q^ - q_ref| of the module's docstring.
    T: lower_factor()'s (n, n) float64; K (R, n) long double, a (R, n) float64, eta (n,) or scalar.  The triangle is exploited: the rows of
    N-tile j meet the columns below 256 (j + 1) only.  -> (q_ref (R,) long double, bound (R,) float64)"""
    n = T.shape[0]
    R = K.shape[0]
    gm = gamma(2 * n + 8)
    absK = np.abs(K).astype(np.float64)
    absKg = absK * (4.0 + 6.0 * a)
    eta = np.broadcast_to(np.asarray(eta, dtype=np.float64), (n,))
    q = np.zeros(R, dtype=LD)
    bound = np.zeros(R)
    for r0 in range(0, n, TILE):
        c = r0 + TILE
        Tt = T[r0:c, :c]
        z = Tt.astype(LD) @ K[:, :c].T  # (256, R)
        q += (z * z).sum(axis=0)
        absT = np.abs(Tt)
        A, G = absT @ absK[:, :c].T, absT @ absKg[:, :c].T
        e = U * G + gm * (A + U * G) + ((absT @ eta[:c]) + c * TINY)[:, None]
        za = np.abs(z).astype(np.float64)
        bound += (2.0 * za * e + e * e).sum(axis=0) + gm * ((za + e) ** 2).sum(axis=0) + TILE * TINY
    return q, bound


def mean(K, a, v, eta=0.0):
    """mu_ref = k . v in long double and the bound on |mu^ - mu_ref|; v (n,) float64 in the layout of K's columns"""
    n = K.shape[1]
    kv = np.abs(K).astype(np.float64) * np.abs(v)[None, :]
    eta = np.broadcast_to(np.asarray(eta, dtype=np.float64), (n,))
    bound = U * ((4.0 + 6.0 * a) * kv).sum(axis=1) + gamma(n + GEN_KSPLIT_MAX) * kv.sum(axis=1) + (eta * np.abs(v)).sum() + n * TINY
    return K @ v.astype(LD), bound


def real_reference(theta, T, v, X, Xs):
    """Everything of a real predict: T as gple_debug_fit_factor returns it (T[n, k]), v = fit.get(R_INVLBL) (N,).
    -> dict(mean, mean_bound, var, var_bound): long double references and float64 bounds per test point"""
    L = lower_factor(T)
    n = L.shape[0]
    K, a, eta = real_kstar(theta, Xs, X, n)
    q, qb = contraction(L, K, a, eta)
    vp = np.zeros(n)
    vp[:len(X)] = v
    mu, mb = mean(K, a, vp, eta)
    self = real_self(theta)
    return dict(mean=mu, mean_bound=mb, var=self - q, var_bound=qb + 4.0 * U * float(self))


def complex_reference(theta, T, v, X, Xs, n_split):
    """The same for a complex predict: v = fit.get(C_INVLBL) (N,) complex.  The mean k v + k~ conj(v) is, in the embedding, the typed rows
    against [2 Re v; 2 Im v]: Re = s^2 (2 K_R Re v + 2 K_C Im v), Im = s^2 (2 K_C Re v + 2 K_I Im v) — the doubling is exact.
    -> dict(mean (complex pair of long doubles as (re, im)), mean_bound (re, im), var, var_bound)"""
    L = lower_factor(T)
    n, N = L.shape[0], len(X)
    assert n == 2 * n_split
    vp = np.zeros(n)
    vp[:N], vp[n_split:n_split + N] = 2.0 * v.real, 2.0 * v.imag
    q, qb, mu, mb = [], [], [], []
    for K, a, eta in complex_kstar(theta, Xs, X, n_split):
        qq, bb = contraction(L, K, a, eta)
        m, b = mean(K, a, vp, eta)
        q.append(qq), qb.append(bb), mu.append(m), mb.append(b)
    self = complex_self(theta)
    return dict(mean=(mu[0], mu[1]), mean_bound=(mb[0], mb[1]), var=self - (q[0] + q[1]), var_bound=qb[0] + qb[1] + 4.0 * U * float(self))


def ratio(value, ref, bound):
    """max |value - ref| / bound over the rows (the difference is formed in long double)"""
    return float((np.abs(np.asarray(value).astype(LD) - ref) / bound).max())


def factor_residual(T, K):
    """(||L K L^T - I||_max, 50 n u ||K||_1 ||L||_1^2) on the padded system, L = lower_factor(T); K (n, n) the padded Gram matrix in fp64"""
    L = lower_factor(T)
    n = L.shape[0]
    n1 = lambda A: np.abs(A).sum(axis=0).max()
    return float(np.abs(L @ K @ L.T - np.eye(n)).max()), 50.0 * n * U * n1(K) * n1(L) ** 2


def padding_is_identity(T, N, n_split):
    """rows and columns N .. n_split - 1 of every half of the padded factor are the identity's"""
    L = lower_factor(T)
    n = L.shape[0]
    pad = np.concatenate([np.arange(h + N, h + n_split) for h in range(0, n, n_split)])
    E = np.eye(n)
    return bool(np.array_equal(L[pad], E[pad]) and np.array_equal(L[:, pad], E[:, pad]))


def cutoff(mean_abs_sq, mean_abs, var):
    """cutoff_value of gple_kernels.h in fp64, operation by operation, on arrays"""
    with np.errstate(invalid="ignore", divide="ignore"):
        a = mean_abs / np.sqrt(var)
        cubic = (3.0 * 2.0 - 2.0 * a - 1.0) * ((a - 1.0) * (a - 1.0)) / 1.0
    return np.where(mean_abs_sq >= 4.0 * var, 1.0, np.where(mean_abs_sq <= var, 0.0, cubic))
