"""Numpy restatement of the absorbing boundary of the MQCLE run ("The absorbing boundary") for the tests — a helper, not
collected by pytest.  Written from the formulas, not from the device code: a complex absorbing potential -i W(x), a multiple of the identity in
surface space, damps every element pointwise at the MQCLE's own order, rho(x, p) <- exp(-2 W(x) tau / hbar) rho(x, p), split as
M(tau / 2) [k steps] M(tau / 2) with M: rho_i. <- (1 - g_i) rho_i., g_i = 1 - exp(-W(x_i) tau / hbar), tau = k dt; what a mask removes is
booked as g_i rho^adia_aa(x_i, p_j) per side of the box, surface a and momentum index j.  rho: (num_pes, num_pes, n_x, n_p) complex, diabatic."""
import functools

import numpy as np

from tests import mqcl_numpy as MN

HBAR = 1.0
PPL_LIM = 1e-4


def absorb(rho, bases, g, n_left):
    """One half-mask: the masked state, every stored double times (1.0 - g) of its row, and the sums [side][a][j] of g_i rho^adia_aa(x_i, p_j)
    over the rows i < n_left (side 0) and the others (side 1), rows with g = 0 left out, in ascending row order"""
    num_pes, n = rho.shape[0], rho.shape[2]
    keep = 1.0 - g
    masked = np.ascontiguousarray(rho).view(np.float64).reshape(num_pes, num_pes, n, rho.shape[3], 2) * keep[None, None, :, None, None]
    masked = np.ascontiguousarray(masked).view(np.complex128).reshape(rho.shape)
    adia = MN.to_basis(rho, bases.C)
    sums = np.zeros((2, num_pes, rho.shape[3]))
    for i in np.flatnonzero(g != 0.0):
        for a in range(num_pes):
            sums[0 if i < n_left else 1, a] += g[i] * adia[a, a, i].real
    return masked, sums


def evolve_absorbing(rho, bases, p, mass, length_x, length_p, dt, n_steps, mask_every, g, n_left, absorbed_p=None, freq=MN.ref_freq):
    """n_steps / mask_every blocks of absorb(g), mask_every Trotter steps, absorb(g) -> the state and the accumulator (a new array)"""
    assert mask_every >= 1 and n_steps % mask_every == 0
    acc = np.zeros((2, rho.shape[0], rho.shape[3])) if absorbed_p is None else np.array(absorbed_p, dtype=np.float64)
    for _ in range(n_steps // mask_every):
        rho, s = absorb(rho, bases, g, n_left)
        acc = acc + s
        rho = MN.evolve(rho, bases, p, mass, length_x, length_p, dt, mask_every, freq)
        rho, s = absorb(rho, bases, g, n_left)
        acc = acc + s
    return rho, acc


def half_mask(w, tau):
    """g = 1 - exp(-W tau / hbar); a W that is not finite absorbs everything"""
    with np.errstate(invalid="ignore", over="ignore"):
        g = -np.expm1(-np.asarray(w, dtype=np.float64) * tau / HBAR)
    return np.where(np.isfinite(w), g, 1.0)


def absorbing_potential(x, mass, xmin, xmax, length):
    """the absorber of the DVR run (pes.cpp:64-93): zero inside (xmin, xmax), x <= xmin on the left-hand branch"""
    c = np.sqrt(2.0) * 1.8540746773013719
    xi = c * np.where(x <= xmin, x - xmin, x - xmax) / length
    w = (2.0 * np.pi * HBAR / length) ** 2 * 2.0 / mass * (1.0 / (c - xi) ** 2 + 1.0 / (c + xi) ** 2 - 2.0 / c ** 2)
    return np.where((x > xmin) & (x < xmax), 0.0, w)


def grid(xmin, xmax, dx, p0, sigma_p, mass, mask_every, dt):
    """The absorbing set-up on a given spacing: the box [xmin, xmax] with int(length / dx) absorber rows a side, length = 2 pi hbar /
    (p0 - 3 sigma_p); x and p by the interpolation rule of main.cpp:89-91, the momentum box p0 +- pi hbar / (2 dx)"""
    length = 2.0 * np.pi * HBAR / (p0 - 3.0 * sigma_p)
    n_abs = int(length / dx)
    n = int((xmax - xmin) / dx) + 1 + 2 * n_abs
    lo, hi = xmin - n_abs * dx, xmax + n_abs * dx
    pmin, pmax = p0 - np.pi * HBAR / dx / 2.0, p0 + np.pi * HBAR / dx / 2.0
    i = np.arange(n, dtype=np.float64)
    x = (lo * (n - 1 - i) + hi * i) / (n - 1)
    p = (pmin * (n - 1 - i) + pmax * i) / (n - 1)
    g = np.clip(half_mask(absorbing_potential(x, mass, xmin, xmax, length), mask_every * dt), 0.0, 1.0)
    return dict(n=n, n_abs=n_abs, x=x, p=p, dx=dx, dp=(pmax - pmin) / (n - 1), length_x=hi - lo, length_p=pmax - pmin, g=g, n_left=int(np.sum(x <= xmin)),
                mass=mass, p0=p0, sigma_p=sigma_p, sigma_x=HBAR / 2.0 / sigma_p, dt=dt, mask_every=mask_every)


def packet(G, bases, x0, num_pes):
    """a normalised Gaussian on the lowest adiabatic surface at (x0, p0) (general.cpp:68-106), as the diabatic state"""
    x, p = G["x"], G["p"]
    w = np.exp(-(((x[:, None] - x0) / G["sigma_x"]) ** 2 + ((p[None, :] - G["p0"]) / G["sigma_p"]) ** 2) / 2.0)
    rho = np.zeros((num_pes, num_pes, len(x), len(p)), dtype=np.complex128)
    rho[0, 0] = w / (w.sum() * G["dx"] * G["dp"])
    return MN.from_basis(rho, bases.C)


class FlatBases:
    """the bases of a constant diagonal potential V = diag(levels): every basis is the identity, no force (what MN.Bases would hold)"""

    def __init__(self, n, levels):
        num_pes = len(levels)
        self.E = np.tile(np.asarray(levels, dtype=np.float64), (n, 1))
        self.C = np.tile(np.eye(num_pes), (n, 1, 1))
        self.lam, self.U = np.zeros((n, num_pes)), self.C.copy()

    def matrix(self, basis):
        return self.C if basis == MN.ADIABATIC else self.U


FLAT_LEVELS = (0.0, 0.01)


@functools.lru_cache(maxsize=None)
def sac_case():
    """The balance case of DESIGN.md §12: SAC, mass 2000, p0 = 10, sigma_p = p0 / 20, box [-5, 5], dx = 0.1 (n = 115, 7 absorber rows a side),
    x0 = 3.5, dt = 1, 25 blocks of 8 steps.  -> (G, bases, the initial state, the final state, the accumulator); computed once per session"""
    G = grid(-5.0, 5.0, 0.1, 10.0, 0.5, 2000.0, 8, 1.0)
    bases = MN.Bases(G["x"], 0, 2)
    rho0 = packet(G, bases, 3.5, 2)
    rho, acc = evolve_absorbing(rho0, bases, G["p"], G["mass"], G["length_x"], G["length_p"], G["dt"], 200, 8, G["g"], G["n_left"])
    return G, bases, rho0, rho, acc


@functools.lru_cache(maxsize=None)
def free_flight_case():
    """The closed-form case of DESIGN.md §12: the flat potential diag(0, 0.01) on the same grid, the packet at x0 = 0, 300 blocks of one step
    dt = 10: everything leaves on the right on surface 0 with the momentum distribution it started with.  Computed once per session"""
    G = grid(-5.0, 5.0, 0.1, 10.0, 0.5, 2000.0, 1, 10.0)
    bases = FlatBases(G["n"], FLAT_LEVELS)
    rho0 = packet(G, bases, 0.0, 2)
    rho, acc = evolve_absorbing(rho0, bases, G["p"], G["mass"], G["length_x"], G["length_p"], G["dt"], 300, 1, G["g"], G["n_left"])
    return G, bases, rho0, rho, acc


def run(rho_dia, bases, G, n_outputs, output_step, x0, until_absorbed=False):
    """The driver loop on the restatement: per output one evolve_absorbing of output_step steps and one observe; records of (t, averages,
    populations, absorbed (2, num_pes)), the stop (None: ran out of outputs), the final state and the accumulator"""
    acc = np.zeros((2, rho_dia.shape[0], rho_dia.shape[3]))
    records, stop = [], None
    last_x = MN.observe(rho_dia, bases, G["x"], G["p"], G["mass"], G["dx"], G["dp"])[1][1]
    for k in range(1, n_outputs + 1):
        rho_dia, acc = evolve_absorbing(rho_dia, bases, G["p"], G["mass"], G["length_x"], G["length_p"], G["dt"], output_step, G["mask_every"], G["g"],
                                        G["n_left"], acc)
        _, av, pops = MN.observe(rho_dia, bases, G["x"], G["p"], G["mass"], G["dx"], G["dp"])
        records.append(dict(t=k * output_step * G["dt"], E=av[0], x=av[1], p=av[2], populations=pops, absorbed=acc.sum(axis=2) * G["dx"] * G["dp"]))
        if pops.sum() < PPL_LIM:
            stop = "absorbed"
        elif not until_absorbed and av[1] > 0 and ((av[1] - last_x) * G["p0"] < 0 or av[1] > -x0):
            stop = "criterion"
        if stop:
            break
        last_x = av[1]
    return records, stop, rho_dia, acc
