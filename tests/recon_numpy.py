"""Independent numpy restatement of the reconstruction experiment of the reference (test/main_evolve.cpp:56-179, test/gpr.cpp) for the tests — a
helper, not collected by pytest.  Written from the formulas in numpy longdouble: the real planes of a state (SuperMatrix, test/io.cpp:25-72
without read_density's averaging), the survey (gpr.cpp:42-82, 119-135, 197-210, 247), generate_training_set (gpr.cpp:215-291) on the
library's Philox draws, the NOCROSS Gram (gpr.cpp:323-326, 384-392) and predict_phase / mean_squared_error (gpr.cpp:654-706, 994-1005).
Adiabatic energies come from the caller (tests/mqcl_numpy.Bases)."""
import numpy as np

from oracle.evolve_oracle import philox4x32

LD = np.longdouble
EPS = 2.0 ** -53
SELECT_TAG = 0x5E1EC7


def planes_of(rho):
    """(num_pes, num_pes, nx, np) complex -> (num_pes^2, nx, np) real planes: (i, i) = Re rho_ii, (i, j > i) = Re rho_ij, (j > i, i) = Im rho_ij"""
    n = rho.shape[0]
    out = np.empty((n * n,) + rho.shape[2:])
    for r in range(n):
        for c in range(n):
            out[r * n + c] = rho[r, c].real if r <= c else rho[c, r].imag
    return out


def is_diagonal(q, num_pes):
    return q // num_pes == q % num_pes


def survey(rho, x, p, mass, dx, dp, energies):
    """-> (values (nq, 7) longdouble: max, min, sum |v|, argmax or -1, population, potential, kinetic; magnitudes (nq, 7): sum of |terms| of every sum)"""
    num_pes = rho.shape[0]
    pl = planes_of(rho)
    val, mag = np.zeros((len(pl), 7), dtype=LD), np.zeros((len(pl), 7), dtype=LD)
    kin = (p.astype(LD) ** 2 / 2 / LD(mass))[None, :]
    for q, v in enumerate(pl):
        vl = v.astype(LD)
        val[q, 0], val[q, 1], val[q, 2] = v.max(), v.min(), np.abs(vl).sum()
        mag[q, 2] = val[q, 2]
        val[q, 3] = int(np.argmax(v)) if v.max() > 0.0 else -1  # numpy's argmax is the first maximum in row-major order
        if is_diagonal(q, num_pes):
            e = energies[:, q // num_pes].astype(LD)[:, None]
            val[q, 4], val[q, 5], val[q, 6] = vl.sum() * dx * dp, (vl * e).sum() * dx * dp, (vl * kin).sum() * dx * dp
            mag[q, 4], mag[q, 5], mag[q, 6] = np.abs(vl).sum() * dx * dp, np.abs(vl * e).sum() * dx * dp, np.abs(vl * kin).sum() * dx * dp
    return val, mag


def uniforms(q, seed, k0, k1):
    """the two uniforms of the draws k0 .. k1 - 1 of plane q: unit53 of words (0, 1) and (2, 3) of Philox4x32-10, counter (k, q, tag, 0), key = seed"""
    k = np.arange(k0, k1, dtype=np.uint64)
    ctr = np.stack([k, np.full_like(k, q), np.full_like(k, SELECT_TAG), np.zeros_like(k)], axis=-1)
    w = philox4x32(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)).astype(np.uint64)
    unit = lambda hi, lo: (((hi << np.uint64(32)) | lo) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
    return unit(w[:, 0], w[:, 1]), unit(w[:, 2], w[:, 3])


def running_sum(plane):
    """P(c): the longdouble running sum of |v| in row-major order"""
    return np.cumsum(np.abs(plane.astype(LD)).ravel())


def weighted_cells(P, u):
    """the first cell whose running sum exceeds u_k = u W (acc_weight < 0, gpr.cpp:251-263), W = P[-1]"""
    return np.searchsorted(P, u.astype(LD) * P[-1], side="right")


def uniform_cells(u, u2, nx, np_):
    return np.floor(u * nx).astype(np.int64) * np_ + np.floor(u2 * np_).astype(np.int64)


def select_from_draws(cells, n_select):
    """the std::set loop of gpr.cpp:236-265 on a given draw sequence: (sorted distinct cells of the first K draws, K), K minimal"""
    seen = set()
    for k, c in enumerate(cells):
        seen.add(int(c))
        if len(seen) == n_select:
            return np.array(sorted(seen)), k + 1
    raise ValueError("not enough draws")


def gram(hyper, A, B, dtype=LD):
    """w_g^2 exp(-(a_x dx)^2 / 2 - (a_p dp)^2 / 2) between the points A (n, 2) and B (m, 2): the ARD kernel alone (no noise off the training set)"""
    _, wg, ax, ap = [dtype(h) for h in hyper]
    A, B = A.astype(dtype), B.astype(dtype)
    d0, d1 = ax * (A[:, None, 0] - B[None, :, 0]), ap * (A[:, None, 1] - B[None, :, 1])
    return wg * wg * np.exp(-(d0 * d0 + d1 * d1) / 2)


def train_gram(hyper, X, dtype=LD):
    return gram(hyper, X, X, dtype) + dtype(hyper[0]) ** 2 * np.eye(len(X), dtype=dtype)


def tables(hyper, X, b, x, p, c=1.0, dtype=LD):
    """Ax (nx, N) = c w_g^2 b_i exp(-(a_x (x_a - X_i))^2 / 2), Ep (np, N) = exp(-(a_p (p_b - P_i))^2 / 2), and the two exponent magnitudes"""
    _, wg, ax, ap = [dtype(h) for h in hyper]
    gx = (ax * (x.astype(dtype)[:, None] - X[:, 0].astype(dtype)[None, :])) ** 2 / 2
    gp = (ap * (p.astype(dtype)[:, None] - X[:, 1].astype(dtype)[None, :])) ** 2 / 2
    return dtype(c) * wg * wg * b.astype(dtype)[None, :] * np.exp(-gx), np.exp(-gp), gx, gp


def predict_plane(hyper, X, b, x, p, c=1.0):
    """c k((x_a, p_b), X) b on the tensor grid in longdouble, and the entry bound 4 eps [(N + 8) S + S_A] + eps max|mu| of the issue"""
    Ax, Ep, gx, gp = tables(hyper, X, b, x, p, c)
    mu = Ax @ Ep.T
    A64, E64 = np.abs(Ax).astype(np.float64), Ep.astype(np.float64)
    S = A64 @ E64.T
    S_A = (A64 * gx.astype(np.float64)) @ E64.T + A64 @ (E64 * gp.astype(np.float64)).T
    tol = 4 * EPS * ((len(X) + 8) * S + S_A) + EPS * float(np.abs(mu).max())
    return mu, tol


def sums_of(mu, v, energy_i, p, mass, dx, dp, diagonal):
    """the six sums of gple_grid_reconstruct for one plane from a prediction mu (already scaled) and the exact plane v, and the |terms| sums"""
    mu, v = mu.astype(LD), v.astype(LD)
    val, mag = np.zeros(6, dtype=LD), np.zeros(6, dtype=LD)
    val[0], val[4], val[5] = ((mu - v) ** 2).sum(), (mu * mu).sum(), (mu * v).sum()
    mag[0], mag[4], mag[5] = val[0], val[4], np.abs(mu * v).sum()
    if diagonal:
        e, kin = energy_i.astype(LD)[:, None], (p.astype(LD) ** 2 / 2 / LD(mass))[None, :]
        val[1], val[2], val[3] = mu.sum() * dx * dp, (mu * e).sum() * dx * dp, (mu * kin).sum() * dx * dp
        mag[1], mag[2], mag[3] = np.abs(mu).sum() * dx * dp, np.abs(mu * e).sum() * dx * dp, np.abs(mu * kin).sum() * dx * dp
    return val, mag


def sums_tolerance(mu, v, tol, energy_i, p, mass, dx, dp, diagonal):
    """what an entry error of tol does to each of the six sums (first order plus the square), for the propagated part of the sums' tolerance"""
    mu, v, tol = mu.astype(np.float64), v.astype(np.float64), np.broadcast_to(tol, mu.shape)
    out = np.zeros(6)
    out[0] = (2 * np.abs(mu - v) * tol + tol * tol).sum()
    out[4] = (2 * np.abs(mu) * tol + tol * tol).sum()
    out[5] = (np.abs(v) * tol).sum()
    if diagonal:
        out[1] = tol.sum() * dx * dp
        out[2] = (tol * np.abs(energy_i)[:, None]).sum() * dx * dp
        out[3] = (tol * (p ** 2 / 2 / mass)[None, :]).sum() * dx * dp
    return out
