"""Independent numpy restatement of the exact MQCLE solver (liouville_equation/ of the reference) for the tests — a helper, not collected by
pytest.  Written from the reference text: basis_transform (pes.cpp:360-700), quantum_liouville_propagation (general.cpp:171-209),
classical_position_liouville_propagator (:266-380), classical_momentum_liouville_propagator (:388-510), the step of main.cpp:192-260 and
calculate_average / calculate_population (general.cpp:108-164).  Every one of the num_pes^2 elements is shifted with np.fft and the
reference's frequency map, and every sub-step hermitises literally (matrix.cpp:414-428).  Potentials and adiabatic states come from
oracle/evolve_oracle_n.py, force bases from numpy.linalg.eigh.  rho: (num_pes, num_pes, n_x, n_p) complex."""
import numpy as np

from oracle import evolve_oracle_n as ON

HBAR = 1.0
PI = np.pi
DIABATIC, ADIABATIC, FORCE = 0, 1, 2


def ref_freq(n):
    """general.cpp:339-346: bin k has frequency k for k < n / 2 (integer division), else k - n"""
    k = np.arange(n)
    return np.where(k < n // 2, k, k - n)


def fftfreq(n):
    return np.rint(np.fft.fftfreq(n) * n).astype(int)


def hermitize(rho):
    """ComplexMatrix::hermitize at every grid point (matrix.cpp:414-428)"""
    out = rho.copy()
    num_pes = rho.shape[0]
    for i in range(num_pes):
        for j in range(i, num_pes):
            re = (rho[i, j].real + rho[j, i].real) / 2.0
            im = (rho[i, j].imag - rho[j, i].imag) / 2.0
            out[i, j] = re + 1j * im
            out[j, i] = re - 1j * im
    return out


class Bases:
    """per-x adiabatic energies E (n, NP) and states C (n, NP, NP; columns), force eigenvalues lam and eigenvectors U"""

    def __init__(self, x, model, num_pes):
        self.E, self.C, _, _ = ON.adiabatic(x, model, num_pes)
        _, Fd = ON.diabatic(x, model, num_pes)
        self.lam, self.U = np.linalg.eigh(Fd)

    def matrix(self, basis):
        return self.C if basis == ADIABATIC else self.U


def to_basis(rho, B):
    """rho(basis) = B^T rho B per grid point (pes.cpp: diabatic_to_*), hermitised"""
    return hermitize(np.einsum("ica,cdij,idb->abij", B, rho, B, optimize=True))


def from_basis(rho, B):
    """rho(dia) = B rho B^T per grid point (pes.cpp: *_to_diabatic), hermitised"""
    return hermitize(np.einsum("iac,cdij,ibd->abij", B, rho, B, optimize=True))


def transform(rho, bases, frm, to):
    """basis_transform[frm][to]: adiabatic <-> force goes through the diabatic basis"""
    if frm == to:
        return rho
    if frm != DIABATIC:
        rho = from_basis(rho, bases.matrix(frm))
    if to != DIABATIC:
        rho = to_basis(rho, bases.matrix(to))
    return rho


def quantum(rho, bases, t):
    """general.cpp:184-209"""
    rho = transform(rho, bases, DIABATIC, ADIABATIC)
    num_pes = rho.shape[0]
    for a in range(num_pes):
        for b in range(a + 1, num_pes):
            dE = bases.E[:, b] - bases.E[:, a]
            rho[a, b] *= np.exp(dE * t / HBAR * 1j)[:, None]
            rho[b, a] *= np.exp(-dE * t / HBAR * 1j)[:, None]
    return transform(rho, bases, ADIABATIC, DIABATIC)


def shift(v, theta, axis, freq):
    """FFT along axis, multiply bin k by exp(i theta(f_k)), inverse FFT with 1/n (MKL backward scale)"""
    n = v.shape[axis]
    f = freq(n)
    th = theta(f)
    return np.fft.ifft(np.fft.fft(v, axis=axis) * np.exp(1j * th), axis=axis)


def position(rho, p, mass, length_x, t, freq=ref_freq):
    """general.cpp:266-380: exp(-p / m 2 f pi i / L_x t) along x for every p column, every element, then hermitise"""
    out = np.empty_like(rho)
    num_pes = rho.shape[0]
    theta = lambda f: -p[None, :] / mass * 2 * f[:, None] * PI / length_x * t  # (k, j)
    for a in range(num_pes):
        for b in range(num_pes):
            out[a, b] = shift(rho[a, b], theta, 0, freq)
    return hermitize(out)


def momentum(rho, bases, length_p, t, freq=ref_freq):
    """general.cpp:388-510: to the force basis, exp(-(lam_a + lam_b) f pi i / L_p t) along p for every x row, hermitise, back"""
    rho = transform(rho, bases, DIABATIC, FORCE)
    out = np.empty_like(rho)
    num_pes = rho.shape[0]
    for a in range(num_pes):
        for b in range(num_pes):
            s = bases.lam[:, a] + bases.lam[:, b]
            theta = lambda f: -s[:, None] * f[None, :] * PI / length_p * t  # (i, k)
            out[a, b] = shift(rho[a, b], theta, 1, freq)
    return transform(hermitize(out), bases, FORCE, DIABATIC)


def step(rho, bases, p, mass, length_x, length_p, dt, freq=ref_freq):
    """one Trotter step of main.cpp:192-260 in the diabatic basis"""
    rho = quantum(rho, bases, dt / 2.0)
    rho = position(rho, p, mass, length_x, dt / 2.0, freq)
    rho = momentum(rho, bases, length_p, dt, freq)
    rho = position(rho, p, mass, length_x, dt / 2.0, freq)
    return quantum(rho, bases, dt / 2.0)


def evolve(rho, bases, p, mass, length_x, length_p, dt, n_steps, freq=ref_freq):
    for _ in range(n_steps):
        rho = step(rho, bases, p, mass, length_x, length_p, dt, freq)
    return rho


# A mass or a momentum box this large takes every R or P phase below the spacing of doubles at 1: that propagator is the identity and the rows
# or columns it would have coupled evolve on their own, which is what makes a restatement at n = 4096 affordable (Tests)
DECOUPLE = 1e300


def evolve_rows(rho_rows, x_rows, p, model, num_pes, length_x, length_p, dt, n_steps, freq=ref_freq):
    """mass = DECOUPLE, so R is the identity: the x rows x_rows alone, rho_rows = rho[:, :, I, :] with every p, are the exact restatement of
    those rows of the full grid"""
    return evolve(rho_rows, Bases(x_rows, model, num_pes), p, DECOUPLE, length_x, length_p, dt, n_steps, freq)


def evolve_columns(rho_cols, bases, p_cols, mass, length_x, dt, n_steps, freq=ref_freq):
    """length_p = DECOUPLE, so P is the identity: the p columns p_cols alone, rho_cols = rho[:, :, :, J] with every x (bases of the full x grid),
    are the exact restatement of those columns of the full grid"""
    return evolve(rho_cols, bases, p_cols, mass, length_x, DECOUPLE, dt, n_steps, freq)


def psi_multiplier(theta, n, freq=ref_freq):
    """the hermitised shift as one multiplier on the stored triangle: psi_k = (phi_k + conj(phi_{(n - k) mod n})) / 2"""
    f = freq(n)
    phi = np.exp(1j * theta(f))
    return 0.5 * (phi + np.conj(phi[(-np.arange(n)) % n]))


def observe(rho_dia, bases, x, p, mass, dx, dp):
    """the adiabatic rho, (E, x, p) and populations of calculate_average / calculate_population (general.cpp:108-164)"""
    adia = transform(rho_dia, bases, DIABATIC, ADIABATIC)
    num_pes = rho_dia.shape[0]
    ppl = np.stack([adia[a, a].real for a in range(num_pes)])  # (a, i, j)
    E = sum((ppl[a] * (bases.E[:, a][:, None] + p[None, :] ** 2 / 2.0 / mass)).sum() for a in range(num_pes)) * dx * dp
    X = (ppl.sum(axis=0) * x[:, None]).sum() * dx * dp
    P = (ppl.sum(axis=0) * p[None, :]).sum() * dx * dp
    pops = ppl.sum(axis=(1, 2)) * dx * dp
    return adia, np.array([E, X, P]), pops


def random_hermitian(num_pes, n, rng):
    """a random Hermitian rho with content at every frequency"""
    r = rng.standard_normal((num_pes, num_pes, n, n)) + 1j * rng.standard_normal((num_pes, num_pes, n, n))
    r = 0.5 * (r + np.conj(np.swapaxes(r, 0, 1)))
    for a in range(num_pes):
        r[a, a] = r[a, a].real
    return np.ascontiguousarray(r)
