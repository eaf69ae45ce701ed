"""numpy restatement of gple_hop_bin_mf / gple_hop_density_mf (csrc/gple_hop.hip, include/gple.h, DESIGN.md §17 "The ensemble in phase space, from
the amplitudes"), on the restatement of the mixed density (tests/hop_density_numpy.py: its cells, with the surface clause dropped, and its
amplitudes).

    cells(state, grid, bin_all)          who is selected (by status alone), and the cell of everyone selected (-1: outside)
    bin_mf(potential, state, grid, ...)  the int64 acc, built with np.add.at: weight planes, coherence planes, the two tallies
    density_mf(acc, N, grid, n_norm)     the complex (N, N, n_x, n_p) density of such an acc
    NumpyHopDensityMfApi                 NumpyMfApi with pes_adiabatic_n, hop_bin / hop_density and hop_bin_mf / hop_density_mf, for
                                         hopping.run(phase_grid=..., phase_density=...); every call is recorded

grid is the 6-tuple (x_first, dx, n_x, p_first, dp, n_p)."""
import numpy as np

from tests import hop_density_numpy as HD
from tests import hop_mf_numpy as HM
from tests import hop_numpy as HN

TWO32 = HD.TWO32
planes, words = HD.planes, HD.words


def cells(state, grid, bin_all=False):
    """HD.cells without the surface clause: a surface in range for everyone, whatever the state carries (a mean-field ensemble passes none)"""
    x, p, b, _, status = state
    return HD.cells((x, p, b, np.zeros(len(np.asarray(status)), dtype=np.int32), status), grid, bin_all)


def bin_mf(potential, state, grid, bin_all=False, acc=None):
    """gple_hop_bin_mf -> acc (a given acc is added to, on a copy)"""
    N = state[2].shape[1]
    n_cells = int(grid[2]) * int(grid[5])
    acc = np.zeros(words(N, grid), dtype=np.int64) if acc is None else np.array(acc, dtype=np.int64)
    assert acc.shape == (words(N, grid),)
    selected, cell = cells(state, grid, bin_all)
    on = cell >= 0
    where = cell[on]
    if on.any():
        c = HD.amplitudes(potential, tuple(np.asarray(v)[on] for v in state))  # formed for the binned ones only, as on the device
        for a in range(N):
            w = c[:, a].real * c[:, a].real + c[:, a].imag * c[:, a].imag
            np.add.at(acc, a * n_cells + where, np.rint(TWO32 * w).astype(np.int64))
        at = N * n_cells
        for k in range(N):
            for l in range(k + 1, N):
                term = c[:, k] * np.conj(c[:, l])
                np.add.at(acc, at + where, np.rint(TWO32 * term.real).astype(np.int64))
                np.add.at(acc, at + n_cells + where, np.rint(TWO32 * term.imag).astype(np.int64))
                at += 2 * n_cells
    acc[-2] += on.sum()
    acc[-1] += (selected & ~on).sum()
    return acc


def density_mf(acc, N, grid, n_norm):
    """gple_hop_density_mf: HD.density with the diagonal scaled as the coherences are, sum 2^-32 / w"""
    n_x, n_p = int(grid[2]), int(grid[5])
    n_cells = n_x * n_p
    rho = HD.density(acc, N, grid, n_norm).reshape(N, N, n_cells)
    acc = np.asarray(acc, dtype=np.int64)
    w = np.float64(n_norm) * np.float64(grid[1]) * np.float64(grid[4])
    for a in range(N):
        rho[a, a] = acc[a * n_cells:(a + 1) * n_cells].astype(np.float64) * (1.0 / TWO32) / w
    return rho.reshape(N, N, n_x, n_p)


class NumpyHopDensityMfApi(HM.NumpyMfApi):
    """NumpyMfApi with the adiabatic energies hopping.run sizes its momentum axis with, the mixed density and the density from the amplitudes"""

    def pes_adiabatic_n(self, num_pes, model, x):
        self.calls.append(("adiabatic",))
        _, E, _, F = HN.states(np.asarray(x, dtype=np.float64), self._potential(num_pes, model))
        return E, F

    @staticmethod
    def _narrow(state):
        return (state[0].astype(np.float64), state[1].astype(np.float64), state[2].astype(np.complex128), state[3], state[4])

    def hop_bin(self, num_pes, model, state, grid, acc=None, bin_all=False):
        self.calls.append(("bin",))
        return HD.bin(self._potential(num_pes, model), self._narrow(state), grid, bin_all, acc)

    def hop_density(self, num_pes, grid, acc, n_norm):
        self.calls.append(("density",))
        return HD.density(acc, num_pes, grid, n_norm)

    def hop_bin_mf(self, num_pes, model, state, grid, acc=None, bin_all=False):
        self.calls.append(("bin_mf",))
        return bin_mf(self._potential(num_pes, model), self._narrow(state), grid, bin_all, acc)

    def hop_density_mf(self, num_pes, grid, acc, n_norm):
        self.calls.append(("density_mf",))
        return density_mf(acc, num_pes, grid, n_norm)
