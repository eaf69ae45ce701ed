"""numpy restatement of the coupled-channel scattering solver of csrc/gple_scatter.hip (gple_scatter, include/gple.h): the
renormalised Numerov march from the transmitted side, operation for operation, vectorised over energies and generic in dtype (float64, and
numpy.longdouble with its complex type).  numpy.linalg has no long double: the inverses are the explicit adjugates of the device, written on the
unique entries of a symmetric matrix, and the eigen-systems of the two ends are the cyclic Jacobi of tests/hop_numpy.py.

    march(potential, num_pes, mass, x_left, x_right, n_steps, energies, dtype)   -> dict(prob, defect, u_left, u_right, eps_left, eps_right)
    NumpyScatterApi                                                             Api.scatter and Api.format_g on this restatement, for scattering.run
    eckart_transmission(k, V0, a, mass)                                         the closed form of V0 sech^2(a x)

A potential is a function of tests/hop_numpy.py (builtin(), table()) or any x (m,) -> V (m, N, N) or (V, anything): V is evaluated in x's dtype.
"""
import numpy as np

from tests import hop_numpy as HN

HBAR = 1.0


def _pairs(N):
    return [(i, j) for i in range(N) for j in range(i, N)]


def sym_inverse(A):
    """The inverse of a symmetric N x N matrix (N = 2, 3) given as {(i, j): array, i <= j}, real or complex, by its adjugate on the unique
    entries: the result is exactly symmetric.  The reciprocal of a complex determinant is conj(det) (1 / |det|^2), one division."""
    N = 2 if (1, 2) not in A else 3
    if N == 2:
        a, b, d = A[0, 0], A[0, 1], A[1, 1]
        det = a * d - b * b
        cof = {(0, 0): d, (0, 1): -b, (1, 1): a}
    else:
        a00, a01, a02, a11, a12, a22 = A[0, 0], A[0, 1], A[0, 2], A[1, 1], A[1, 2], A[2, 2]
        cof = {(0, 0): a11 * a22 - a12 * a12, (0, 1): a02 * a12 - a01 * a22, (0, 2): a01 * a12 - a02 * a11,
               (1, 1): a00 * a22 - a02 * a02, (1, 2): a01 * a02 - a00 * a12, (2, 2): a00 * a11 - a01 * a01}
        det = a00 * cof[0, 0] + a01 * cof[0, 1] + a02 * cof[0, 2]
    if np.iscomplexobj(det):
        r = np.conj(det) * (1.0 / (det.real * det.real + det.imag * det.imag))
    else:
        r = 1.0 / det
    return {k: c * r for k, c in cof.items()}


def _at(S, i, j):
    return S[i, j] if i <= j else S[j, i]


def _values(potential, x):
    out = potential(x)
    return out[0] if isinstance(out, tuple) else out


def asymptote(eps, E, c, ctype):
    """Per channel of one end: u = 12 / (1 - t) - 10 with t = c (eps - E), the root z of z + 1 / z = u that moves or decays to the right
    (complex), s = Im z (positive exactly for an open channel) and 1 / z"""
    one = eps.dtype.type(1)
    t = c * (eps - E[:, None])
    u = 12.0 / (one - t) - 10.0
    half = u / 2.0
    is_open = np.abs(u) < 2.0
    with np.errstate(invalid="ignore", divide="ignore"):
        zi = np.where(is_open, np.sqrt(np.where(is_open, (one - half) * (one + half), one)), 0 * u)
        a = np.abs(half)
        r = a + np.sqrt(np.where(is_open, one, (a - one) * (a + one)))
        zr = np.where(is_open, half, np.copysign(one / r, u))
    z = (zr + 1j * zi).astype(ctype)
    zinv = np.conj(z) * (one / (zr * zr + zi * zi))
    return u, z, zi, zinv


def march(potential, num_pes, mass, x_left, x_right, n_steps, energies, dtype=np.float64):
    """gple_scatter on the restatement.  prob (n_E, incoming i, side: 0 reflected 1 transmitted, final j), defect (n_E, i); the columns of a
    closed incoming channel are NaN, a closed final channel is exactly 0.  u_left, u_right (n_E, N): the u_j of both ends (|u| = 2 is a threshold)"""
    dtype = np.dtype(dtype)
    ty, ctype = dtype.type, HN.complex_of(dtype)
    N, n_steps = int(num_pes), int(n_steps)
    E = np.atleast_1d(np.asarray(energies)).astype(dtype)
    nE = len(E)
    x_left, x_right, mass = ty(x_left), ty(x_right), ty(mass)
    h = (x_right - x_left) / ty(n_steps)
    c = h * h / ty(12) * (ty(2) * mass / ty(HBAR * HBAR))
    x = x_left + np.arange(n_steps + 1).astype(dtype) * h
    V = np.asarray(_values(potential, x), dtype=dtype)  # (n_steps + 1, N, N)
    pairs = _pairs(N)
    eps_l, C_l = HN.jacobi(V[:1])
    eps_r, C_r = HN.jacobi(V[-1:])
    eps_l, C_l, eps_r, C_r = eps_l[0], C_l[0], eps_r[0], C_r[0]
    u_l, z_l, s_l, zinv_l = asymptote(eps_l[None, :], E, c, ctype)
    u_r, z_r, s_r, zinv_r = asymptote(eps_r[None, :], E, c, ctype)
    # L_{N+1} = C_R diag(1 / z^R) C_R^T
    L = {}
    for (i, j) in pairs:
        acc = np.zeros(nE, dtype=ctype)
        for k in range(N):
            acc = acc + (C_r[i, k] * C_r[j, k]) * zinv_r[:, k]
        L[i, j] = acc
    M = None
    one = ty(1)
    for n in range(n_steps, -1, -1):
        G = sym_inverse(L)
        if n < n_steps:
            if M is None:
                M = {(i, j): _at(G, i, j) for i in range(N) for j in range(N)}  # I G
            else:
                new = {}
                for i in range(N):
                    for j in range(N):
                        acc = M[i, 0] * _at(G, 0, j)
                        for k in range(1, N):
                            acc = acc + M[i, k] * _at(G, k, j)
                        new[i, j] = acc
                M = new
        A = {}
        for (i, j) in pairs:
            A[i, j] = one - c * (V[n, i, i] - E) if i == j else np.full(nE, -(c * V[n, i, j]), dtype=dtype)
        Ainv = sym_inverse(A)
        L = {(i, j): (12.0 * Ainv[i, j] - 10.0 if i == j else 12.0 * Ainv[i, j]) - G[i, j] for (i, j) in pairs}
    # the match at the left: Lambda = C_L^T L_0 C_L
    P = {(k, j): sum((_at(L, k, l) * C_l[l, j] for l in range(1, N)), _at(L, k, 0) * C_l[0, j]) for k in range(N) for j in range(N)}
    Lam = {(i, j): sum((C_l[k, i] * P[k, j] for k in range(1, N)), C_l[0, i] * P[0, j]) for (i, j) in pairs}
    B = {(i, j): (z_l[:, i] - Lam[i, j] if i == j else -Lam[i, j]) for (i, j) in pairs}
    Binv = sym_inverse(B)
    rhs = {(i, j): (Lam[i, j] - zinv_l[:, i] if i == j else Lam[i, j]) for (i, j) in pairs}
    rho = {(i, j): sum((_at(Binv, i, k) * _at(rhs, k, j) for k in range(1, N)), _at(Binv, i, 0) * _at(rhs, 0, j)) for i in range(N) for j in range(N)}
    W = {(i, j): (rho[i, j] + one if i == j else rho[i, j]) for i in range(N) for j in range(N)}  # I + rho
    Q = {(i, j): sum((C_l[i, k] * W[k, j] for k in range(1, N)), C_l[i, 0] * W[0, j]) for i in range(N) for j in range(N)}
    Y = {(i, j): sum((M[i, k] * Q[k, j] for k in range(1, N)), M[i, 0] * Q[0, j]) for i in range(N) for j in range(N)}
    tau = {(i, j): sum((C_r[k, i] * Y[k, j] for k in range(1, N)), C_r[0, i] * Y[0, j]) for i in range(N) for j in range(N)}
    prob = np.zeros((nE, N, 2, N), dtype=dtype)
    defect = np.zeros((nE, N), dtype=dtype)
    nan = ty(np.nan)
    for i in range(N):
        open_i = s_l[:, i] > 0
        total = np.zeros(nE, dtype=dtype)
        with np.errstate(invalid="ignore", divide="ignore"):
            for side, (amp, s_out) in enumerate(((rho, s_l), (tau, s_r))):
                for j in range(N):
                    a = amp[j, i]
                    p = s_out[:, j] * (a.real * a.real + a.imag * a.imag) / s_l[:, i]
                    p = np.where(s_out[:, j] > 0, p, np.zeros(nE, dtype=dtype))
                    prob[:, i, side, j] = np.where(open_i, p, nan)
                    total = total + p
        defect[:, i] = np.where(open_i, total - one, nan)
    return dict(prob=prob, defect=defect, u_left=u_l, u_right=u_r, eps_left=eps_l, eps_right=eps_r)


def near_threshold(result, margin=1e-9):
    """the energies (a mask) for which some |u_j| - 2 of either end lies within margin of zero"""
    u = np.concatenate([result["u_left"], result["u_right"]], axis=1).astype(np.float64)
    return (np.abs(np.abs(u) - 2.0) <= margin).any(axis=1)


def eckart_transmission(k, V0, a, mass):
    """T of V0 sech^2(a x) at wavenumber k (hbar = 1), for 8 m V0 / a^2 > 1"""
    k = np.asarray(k, dtype=np.longdouble)
    pi = 4 * np.arctan(np.longdouble(1))
    sh = np.sinh(pi * k / a) ** 2
    return sh / (sh + np.cosh(pi / 2 * np.sqrt(np.longdouble(8) * mass * V0 / (a * a) - 1)) ** 2)


def format_g(values, per_line, join=False):
    """the text of Api.format_g on the host: "%g" with a blank before every number (join: not before the first of a line)"""
    rows = np.asarray(values, dtype=np.float64).reshape(-1, int(per_line))
    return "".join(("" if join else " ") + " ".join("%g" % v for v in row) + "\n" for row in rows).encode()


class NumpyScatterApi:
    """Api.scatter and Api.format_g on the restatement: potentials = {model id: potential}; a built-in id that is not listed is made on demand"""

    def __init__(self, potentials=None, dtype=np.float64):
        self.potentials, self.dtype = dict(potentials or {}), dtype
        self.calls = []

    def _potential(self, num_pes, model):
        if model not in self.potentials:
            self.potentials[model] = HN.builtin(model, num_pes)
        return self.potentials[model]

    def pes_diabatic_n(self, num_pes, model, x):
        V, F = self._potential(num_pes, model)(np.asarray(x, dtype=np.float64))
        return V, F

    def scatter(self, num_pes, model, mass, x_left, x_right, n_steps, energies, want_defect=True):
        self.calls.append((int(n_steps), len(np.atleast_1d(energies))))
        r = march(self._potential(num_pes, model), num_pes, mass, x_left, x_right, n_steps, energies, self.dtype)
        return r["prob"].astype(np.float64), (r["defect"].astype(np.float64) if want_defect else None)

    def format_g(self, values, per_line, lines_per_block=0, join=False):
        return memoryview(format_g(values, per_line, join))
