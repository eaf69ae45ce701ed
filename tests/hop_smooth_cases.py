"""The cases tests/test_gpu_hop_smooth.py and tests/test_hop_smooth_host.py share.  The ensembles are those of tests/hop_outgoing_cases.py: 293
trajectories, seed 0, evolved until some have left on each side and some still run: DAC at p0 = 10 by fewest switches and by Ehrenfest steps,
TSAC from the middle surface, the table of DAC at dx = 1 / 16.  The GPU test evolves them on the device, the host test by the restatements.
Every ensemble goes through both calls (gple_hop_smooth, gple_hop_smooth_mf), with and without GPLE_HOP_BIN_ALL, on five grids laid over it
and with two pairs of bandwidths.

    check(field, tallies, potential, state, ...)  |field - long double| <= B for every entry of every plane and equal tallies -> the worst ratio
"""
import numpy as np

from tests import hop_numpy as HN
from tests import hop_outgoing_cases as HOC
from tests import hop_smooth_numpy as HS

N_TRAJ = HOC.N_TRAJ
ENSEMBLES = {"dac10-fssh": ("dac10", "fssh"), "dac10-ehrenfest": ("dac10", "ehrenfest"), "tsac": ("tsac", "fssh"), "table2": ("table2", "fssh")}
SHAPES = [(24, 40), (64, 64), (65, 17), (1, 33), (16, 1)]
BANDWIDTHS = {"1.5d": (1.5, 1.5), "0.3dx-4dp": (0.3, 4.0)}  # in units of the grid's spacings
FORMS = [(mean_field, bin_all) for mean_field in (False, True) for bin_all in (False, True)]


def grid_over(state, n_x, n_p):
    """n_x x n_p lines from the least to the largest finite x and p of the ensemble; an axis of one line sits at the median, its spacing (which
    only sets the bandwidth) a tenth of the range"""
    axes = []
    for values, n in ((state[0], n_x), (state[1], n_p)):
        v = np.asarray(values, dtype=np.float64)
        v = v[np.isfinite(v)]
        lo, hi = float(v.min()), float(v.max())
        axes += [float(np.median(v)), (hi - lo) / 10.0, n] if n == 1 else [lo, (hi - lo) / (n - 1), n]
    return tuple(axes)


def configurations(state):
    """(label, grid, h) for the five shapes and the two bandwidths"""
    for shape in SHAPES:
        grid = grid_over(state, *shape)
        for label, (f_x, f_p) in BANDWIDTHS.items():
            yield f"{shape[0]}x{shape[1]} h={label}", grid, (f_x * grid[1], f_p * grid[4])


def signs_are_safe(potential, state, mean_field, bin_all):
    """the precondition of a comparison of coherences: at every used x the last non-zero component of every eigenvector column is well away
    from 0, so no two evaluations can choose opposite signs for it"""
    used, _ = HS.selection(state, mean_field, bin_all)
    if not used.any():
        return True
    Cm = HN.states(np.asarray(state[0])[used], potential)[2]
    last = np.zeros((Cm.shape[0], Cm.shape[1]))
    for i in range(Cm.shape[1]):
        last = np.where(Cm[:, i, :] != 0, Cm[:, i, :], last)
    return np.abs(last).min() > 1e-9


_wide = {}


def reference(key, potential, state, grid, h, n_norm, mean_field, bin_all):
    """the long double field with its bound, made once per key and never changed"""
    if key not in _wide:
        rho, tallies, B = HS.smooth(potential, state, grid, h, n_norm, mean_field, bin_all, np.longdouble, True)
        for a in (rho, B):
            a.setflags(write=False)
        _wide[key] = (rho, tallies, B)
    return _wide[key]


def check(field, tallies, key, potential, state, grid, h, n_norm, mean_field, bin_all):
    """asserts the tallies equal and |field - long double| <= B part by part, every entry of every plane -> the worst error over bound"""
    wide, want, B = reference(key, potential, state, grid, h, n_norm, mean_field, bin_all)
    assert tuple(tallies) == tuple(want), (key, tallies, want)
    field = np.asarray(field)
    assert field.dtype == np.complex128 and field.shape == wide.shape
    err = np.stack([np.abs(field.real.astype(np.longdouble) - wide.real), np.abs(field.imag.astype(np.longdouble) - wide.imag)], axis=-1)
    assert np.isfinite(field.view(np.float64)).all(), key
    assert (err <= B).all(), (key, float(np.max(err - B)))
    return float(np.max(np.divide(err, B, out=np.zeros_like(err), where=B > 0)))
