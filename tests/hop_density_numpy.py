"""numpy restatement of gple_hop_bin / gple_hop_density (csrc/gple_hop.hip, include/gple.h, DESIGN.md §17 "The ensemble in phase space"), on the
restatement of the hopping step itself (tests/hop_numpy.py).

    planes(N), words(N, grid)            the planes of an accumulator and its length, the two tallies included
    cells(state, grid, bin_all)          who is selected, and the cell of everyone selected (-1: outside)
    bin(potential, state, grid, ...)     the int64 acc, built with np.add.at
    density(acc, N, grid, n_norm)        the complex (N, N, n_x, n_p) density of an acc
    NumpyHopDensityApi                   NumpyHopApi with hop_bin / hop_density (and pes_adiabatic_n), for hopping.run(phase_grid=...)

grid is the 6-tuple (x_first, dx, n_x, p_first, dp, n_p)."""
import numpy as np

from tests import hop_numpy as HN

TWO32 = 4294967296.0


def planes(N):
    return N + N * (N - 1)


def words(N, grid):
    return planes(N) * int(grid[2]) * int(grid[5]) + 2


def cells(state, grid, bin_all=False):
    """(selected (n,) bool, cell (n,) int64: i_x n_p + i_p of a selected trajectory on the grid, -1 otherwise).  The cell rule of the header: a
    subtraction, one division, one addition, one floor, compared in double (a NaN compares false: outside)"""
    x, p, _, surface, status = state
    x_first, dx, n_x, p_first, dp, n_p = grid
    N = state[2].shape[1]
    surface, status = np.asarray(surface), np.asarray(status)
    selected = (status >= 0) & (status <= 2) & (surface >= 0) & (surface < N) & ((status == 0) | bool(bin_all))
    with np.errstate(invalid="ignore", over="ignore"):
        fx = np.floor((np.asarray(x, dtype=np.float64) - np.float64(x_first)) / np.float64(dx) + 0.5)
        fp = np.floor((np.asarray(p, dtype=np.float64) - np.float64(p_first)) / np.float64(dp) + 0.5)
        inside = selected & (fx >= 0.0) & (fx < float(n_x)) & (fp >= 0.0) & (fp < float(n_p))
    cell = np.full(len(fx), -1, dtype=np.int64)
    cell[inside] = fx[inside].astype(np.int64) * int(n_p) + fp[inside].astype(np.int64)
    return selected, cell


def amplitudes(potential, state):
    """c = C^T b at every trajectory's x, as observe_terms forms it"""
    _, _, C, _ = HN.states(state[0], potential)
    return np.einsum("mik,mi->mk", C, state[2])


def bin(potential, state, grid, bin_all=False, acc=None):
    """gple_hop_bin -> acc (a given acc is added to, on a copy)"""
    N = state[2].shape[1]
    n_cells = int(grid[2]) * int(grid[5])
    acc = np.zeros(words(N, grid), dtype=np.int64) if acc is None else np.array(acc, dtype=np.int64)
    assert acc.shape == (words(N, grid),)
    selected, cell = cells(state, grid, bin_all)
    on = cell >= 0
    where, a = cell[on], np.asarray(state[3])[on].astype(np.int64)
    np.add.at(acc, a * n_cells + where, 1)
    at = N * n_cells
    c = amplitudes(potential, tuple(np.asarray(v)[on] for v in state)) if on.any() else None  # formed for the binned ones only, as on the device
    for k in range(N if on.any() else 0):
        for l in range(k + 1, N):
            term = c[:, k] * np.conj(c[:, l])
            np.add.at(acc, at + where, np.rint(TWO32 * term.real).astype(np.int64))
            np.add.at(acc, at + n_cells + where, np.rint(TWO32 * term.imag).astype(np.int64))
            at += 2 * n_cells
    acc[-2] += on.sum()
    acc[-1] += (selected & ~on).sum()
    return acc


def density(acc, N, grid, n_norm):
    """gple_hop_density: w = n_norm dx dp left to right; count / w; sum 2^-32 / w; the lower planes from the negated sums"""
    n_x, n_p = int(grid[2]), int(grid[5])
    n_cells = n_x * n_p
    acc = np.asarray(acc, dtype=np.int64)
    assert acc.shape == (words(N, grid),)
    w = np.float64(n_norm) * np.float64(grid[1]) * np.float64(grid[4])
    rho = np.zeros((N, N, n_cells), dtype=np.complex128)
    for a in range(N):
        rho[a, a] = acc[a * n_cells:(a + 1) * n_cells].astype(np.float64) / w
    at = N * n_cells
    for a in range(N):
        for b in range(a + 1, N):
            re, im = acc[at:at + n_cells], acc[at + n_cells:at + 2 * n_cells]
            rho[a, b].real = rho[b, a].real = re.astype(np.float64) * (1.0 / TWO32) / w
            rho[a, b].imag = im.astype(np.float64) * (1.0 / TWO32) / w
            rho[b, a].imag = (-im).astype(np.float64) * (1.0 / TWO32) / w
            at += 2 * n_cells
    return rho.reshape(N, N, n_x, n_p)


class NumpyHopDensityApi(HN.NumpyHopApi):
    """NumpyHopApi with the two density calls, and the adiabatic energies hopping.run sizes its momentum axis with"""

    def pes_adiabatic_n(self, num_pes, model, x):
        self.calls.append(("adiabatic",))
        x = np.asarray(x, dtype=np.float64)
        _, E, _, F = HN.states(x, self._potential(num_pes, model))
        return E, F

    def hop_bin(self, num_pes, model, state, grid, acc=None, bin_all=False):
        self.calls.append(("bin",))
        narrow = (state[0].astype(np.float64), state[1].astype(np.float64), state[2].astype(np.complex128), state[3], state[4])
        return bin(self._potential(num_pes, model), narrow, grid, bin_all, acc)

    def hop_density(self, num_pes, grid, acc, n_norm):
        self.calls.append(("density",))
        return density(acc, num_pes, grid, n_norm)
