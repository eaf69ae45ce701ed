"""Independent numpy restatement of the exact DVR dynamics (schrodinger_equation/general.cpp of the reference) for the tests — a helper,
not collected by pytest.  Written from the formulas: Hamiltonian_construction (general.cpp:106-200, no absorbing term), Evolution::evolve
(general.cpp:241-252) and output_phase_space_distribution (general.cpp:324-411).  Potentials from oracle/evolve_oracle_n.py."""
import math

import numpy as np

from oracle import evolve_oracle_n as ON

HBAR = 1.0
REFLECTIVE, PERIODIC = 0, 1


def grid(x_first, dx, n):
    return x_first + dx * np.arange(n)


def hamiltonian(num_pes, model, boundary, x_first, dx, n, mass):
    """H (dim x dim), index m n + a: V on the diagonal grid blocks, kinetic energy on the diagonal surface blocks."""
    x = grid(x_first, dx, n)
    V, _ = ON.diabatic(x, model, num_pes)
    H = np.zeros((num_pes * n, num_pes * n))
    a = np.arange(n)
    for m in range(num_pes):
        for mm in range(num_pes):
            H[m * n + a, mm * n + a] += V[:, m, mm]
    d = a[None, :] - a[:, None]  # column - row
    sign = np.where(d % 2 == 0, 1.0, -1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        if boundary == REFLECTIVE:  # Colbert-Miller
            T = np.where(d == 0, (math.pi * HBAR / dx) ** 2 / 6.0 / mass, sign * (HBAR / dx / np.where(d == 0, 1, d)) ** 2 / mass)
        else:
            L = x[n - 1] - x[0]
            diff = -d * math.pi / n
            T = np.where(d == 0, (math.pi * HBAR / L) ** 2 / 6.0 / mass * (n * n - 1),
                         sign * np.cos(diff) * (math.pi * HBAR / L / np.where(d == 0, 1.0, np.sin(diff))) ** 2 / mass)
    for m in range(num_pes):
        H[m * n:(m + 1) * n, m * n:(m + 1) * n] += T
    return H


def half_range(boundary, n):
    return (n - 1) // 2 if boundary == REFLECTIVE else n // 3


def wigner_table(p, dx, kh):
    """E[b, k + kh] = exp(2 i p_b y_k / hbar) with the argument formed as general.cpp:368 forms it (fp64)."""
    k = np.arange(-kh, kh + 1)
    arg = 2.0 * np.asarray(p)[:, None] * (k * dx)[None, :] / HBAR
    return np.cos(arg) + 1j * np.sin(arg)


def wigner(psi, num_pes, boundary, dx, p, dtype=np.clongdouble):
    """P (num_pes, num_pes, n, n_p) accumulated in `dtype`, and the bound sum_k |psi_i[a-k]| |psi_j[a+k]| (num_pes, num_pes, n)."""
    psi = np.asarray(psi, dtype=np.complex128)
    n = len(psi) // num_pes
    kh = half_range(boundary, n)
    E = wigner_table(p, dx, kh).astype(dtype)
    a = np.arange(n)
    P = np.zeros((num_pes, num_pes, n, len(p)), dtype=dtype)
    bound = np.zeros((num_pes, num_pes, n))
    for i in range(num_pes):
        for j in range(num_pes):
            pi, pj = psi[i * n:(i + 1) * n].astype(dtype), psi[j * n:(j + 1) * n].astype(dtype)
            for k in range(-kh, kh + 1):
                u, v = a - k, a + k
                if boundary == PERIODIC:
                    u, v, ok = u % n, v % n, np.ones(n, bool)
                else:
                    ok = (u >= 0) & (u < n) & (v >= 0) & (v < n)
                    u, v = np.clip(u, 0, n - 1), np.clip(v, 0, n - 1)
                A = np.where(ok, pi[u] * np.conj(pj[v]), 0)
                P[i, j] += A[:, None] * E[None, :, k + kh]
                bound[i, j] += np.where(ok, np.abs(psi[i * n + u]) * np.abs(psi[j * n + v]), 0.0)
    return P * (dx / (math.pi * HBAR)), bound


def wigner_averages(P, x, p, energies, mass, dx):
    """(E, x, p) of general.cpp:393-410 from P (num_pes, num_pes, n, n_p)."""
    num_pes = P.shape[0]
    dp = (p[-1] - p[0]) / (len(p) - 1)
    E = X = Pm = 0.0
    for i in range(num_pes):
        R = P[i, i].real.astype(np.float64)
        rows, cols = R.sum(axis=1), R.sum(axis=0)
        X += np.dot(rows, x)
        E += np.dot(rows, energies[:, i]) + np.dot(cols, np.asarray(p) ** 2 / 2.0 / mass)
        Pm += np.dot(cols, p)
    return np.array([E * dx * dp, X * dx * dp, Pm * dx * dp])


def gaussian(x, x0, p0, sigma_x):
    psi = np.exp(-((x - x0) / 2 / sigma_x) ** 2 + 1j * p0 * x / HBAR)
    dx = x[1] - x[0]
    return psi / math.sqrt(np.vdot(psi, psi).real * dx)


def analytic_wigner(x, p, x0, p0, sigma_x):
    return np.exp(-(x[:, None] - x0) ** 2 / (2 * sigma_x ** 2) - 2 * sigma_x ** 2 * (p[None, :] - p0) ** 2 / HBAR ** 2) / (math.pi * HBAR)


def run_loop(num_pes, model, boundary, s, n_outputs, energies_and_basis):
    """The output loop of main.cpp:210-298 restated (spectral propagation, populations, <E> <x> <p> from psi, Wigner averages, stop criteria):
    records of (t, populations, E, x, p, Wigner E, x, p) up to the stop.  energies_and_basis: (E (n, N), C (n, N, N)) per grid point."""
    n, dx, x, p, mass = s["n_grids"], s["dx"], s["x"], s["p"], s["mass"]
    en, C = energies_and_basis
    H = hamiltonian(num_pes, model, boundary, x[0], dx, n, mass)
    lam, U = np.linalg.eigh(H)
    g = gaussian(x, s["x0"], s["p0"], s["sigma_x"])
    psi0 = np.zeros(num_pes * n, dtype=complex)
    for j in range(num_pes):
        psi0[j * n:(j + 1) * n] = C[:, j, 0] * g
    c0 = U.T @ psi0
    jj = np.arange(n)
    d = jj[:, None] - jj[None, :]
    with np.errstate(divide="ignore"):
        D = np.where(d == 0, 0.0, np.where(d % 2 == 0, 1.0, -1.0) / dx / np.where(d == 0, 1, d))
    out, last_x, old = [], s["x0"], np.zeros(num_pes)
    for k in range(n_outputs):
        t = k * s["dt"]
        psi = U @ (np.exp(-1j * lam * t / HBAR) * c0)
        ad = np.einsum("ajk,ja->ka", C, psi.reshape(num_pes, n)).reshape(-1)
        pops = np.array([np.sum(np.abs(ad[m * n:(m + 1) * n]) ** 2) * dx for m in range(num_pes)])
        E = np.vdot(psi, H @ psi).real * dx
        X = sum(np.dot(x, np.abs(psi[m * n:(m + 1) * n]) ** 2) for m in range(num_pes)) * dx
        Pm = np.vdot(psi, np.concatenate([-1j * HBAR * (D @ psi[m * n:(m + 1) * n]) for m in range(num_pes)])).real * dx
        W, _ = wigner(ad, num_pes, boundary, dx, p, dtype=np.complex128)
        out.append(dict(t=t, populations=pops, E=E, x=X, p=Pm, phase_averages=wigner_averages(W, x, p, en, mass, dx)))
        if X > 0.0 and (X > -s["x0"] or (X - last_x) * s["p0"] < 0 or np.all(np.abs(pops - old) < 1e-5)):
            break
        last_x, old = X, pops
    return out
