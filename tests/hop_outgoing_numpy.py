"""numpy restatement of gple_hop_outgoing, gple_hop_outgoing_mf and gple_hop_outgoing_sqc (csrc/gple_hop.hip, include/gple.h, DESIGN.md §17 "What
left the box"), generic in dtype as the restatements it stands on: float64, and numpy.longdouble for the margins.  The weights and the energies
are read out of the terms those restatements give their sums (hop_numpy, hop_mf_numpy and hop_sqc_numpy.observe_terms); the sums are Python
integers.

    classify(form, potential, state, mass, ...)   per trajectory: who runs, who is skipped, the side, the level or the weights, p and q_E
    bins(q, grid)                                 the bin of every q (-1: outside): the four IEEE operations of the header, in float64
    outgoing(form, potential, state, ...)         the int64 acc
    edge_distance(q, grid)                        how far, in steps, a (long double) q is from the nearest edge between two bins
    Numpy*OutgoingApi                             the stand-in apis of the four methods with the three calls, for hopping.run(outgoing=...)

form is "surface", "amplitude" or "window"; grid is (first, step, n_bins); axis is 0 / "momentum" or 1 / "energy"."""
import numpy as np

from tests import hop_mash_numpy as HA
from tests import hop_mf_numpy as HM
from tests import hop_numpy as HN
from tests import hop_scan_numpy as HS
from tests import hop_sqc_numpy as HQ

TWO32 = 4294967296
FORMS = ("surface", "amplitude", "window")
AXES = {"momentum": 0, "energy": 1, 0: 0, 1: 1}
TALLIES = ("binned", "outside", "running", "unassigned")


def words(N, n_bins):
    return 2 * N * int(n_bins) + 4


def classify(form, potential, state, mass, window=None, gamma=None):
    """dict of (n,) arrays: running (status 0), finished (status 1 or 2 and, form "surface", a surface in range), side (status - 1 where
    finished), level (the one plane of a "surface" or "window" trajectory, -1: none, which with "window" is `unassigned`), w (n, N) the weights
    of "amplitude", p, energy = q_E: the last term of the form's observe_terms"""
    x, p, b, surface, status = state
    N, n = b.shape[1], len(x)
    surface, status = np.asarray(surface).astype(np.int64), np.asarray(status).astype(np.int64)
    finished = (status == 1) | (status == 2)
    level, w = np.full(n, -1, dtype=np.int64), np.zeros((n, N), dtype=x.dtype)
    if form == "surface":
        finished &= (surface >= 0) & (surface < N)
        tame = (x, p, b, np.where(finished, surface, 0), np.where(finished, status, 0))  # observe_terms indexes by both
        terms = HN.observe_terms(potential, tame, mass)
        level = np.where(finished, surface, -1)
    elif form == "amplitude":
        terms = HM.observe_terms(potential, state, mass)
        w = terms[:, N:2 * N] + terms[:, 2 * N:3 * N]  # one of the two is the weights, the other zeros
    elif form == "window":
        terms = HQ.observe_terms(potential, state, mass, window, gamma)
        for k in range(N):
            level = np.where((terms[:, N + k] + terms[:, 2 * N + k]) != 0, k, level)
    else:
        raise ValueError(form)
    return dict(running=status == 0, finished=finished, side=np.where(finished, status - 1, -1), level=level, w=w, p=p, energy=terms[:, -1])


def bins(q, grid):
    """j = floor((q - first) / step + 0.5) in float64, compared with 0 and n_bins in double; -1 where outside (a NaN compares false)"""
    first, step, n_bins = grid
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor((np.asarray(q, dtype=np.float64) - np.float64(first)) / np.float64(step) + 0.5)
        inside = (f >= 0.0) & (f < float(n_bins))
    j = np.full(len(f), -1, dtype=np.int64)
    j[inside] = f[inside].astype(np.int64)
    return j


def edge_distance(q, grid):
    """|t - rint(t)| for t = (q - first) / step + 0.5 in q's dtype: the distance of q to the nearest edge between two bins, in steps"""
    ty = q.dtype.type
    t = (q - ty(grid[0])) / ty(grid[1]) + ty(0.5)
    return np.abs(t - np.rint(t))


def outgoing(form, potential, state, mass, grid, axis, window=None, gamma=None, acc=None, skip=None, parts=None):
    """gple_hop_outgoing (form "surface"), _mf ("amplitude"), _sqc ("window") -> acc, int64 (a given acc is added to, on a copy).  skip: a mask
    of trajectories left out entirely.  parts: a dict that receives classify()'s arrays, the bin j and q of every trajectory"""
    N, n_bins = state[2].shape[1], int(grid[2])
    narrow = (state[0].astype(np.float64), state[1].astype(np.float64), state[2].astype(np.complex128), state[3], state[4])
    c = classify(form, potential, narrow, mass, window, gamma)
    q = c["energy"] if AXES[axis] else c["p"]
    j = bins(q, grid)
    sums = [0] * words(N, n_bins) if acc is None else [int(v) for v in np.asarray(acc, dtype=np.int64)]
    assert len(sums) == words(N, n_bins)
    tally = 2 * N * n_bins
    for i in range(len(j)):
        if skip is not None and skip[i]:
            continue
        if c["running"][i]:
            sums[tally + 2] += 1
        elif not c["finished"][i]:
            continue
        elif form == "window" and c["level"][i] < 0:
            sums[tally + 3] += 1
        elif j[i] < 0:
            sums[tally + 1] += 1
        else:
            plane = int(c["side"][i]) * N * n_bins + int(j[i])
            if form == "amplitude":
                for k in range(N):
                    sums[plane + k * n_bins] += int(np.rint(np.float64(TWO32) * c["w"][i, k]))
            else:
                sums[plane + int(c["level"][i]) * n_bins] += TWO32
            sums[tally] += 1
    if parts is not None:
        parts.update(c, j=j, q=q)
    return np.array(sums, dtype=np.int64)


def widen(state):
    x, p, b, surface, status = state
    return x.astype(np.longdouble), p.astype(np.longdouble), b.astype(np.clongdouble), surface, status


def margins(form, potential, state, mass, grid, axis, window=None, gamma=None):
    """What the long double restatement says of every trajectory of the float64 state: edge (n,) = edge_distance of its q (inf on the momentum
    axis, where q is the stored p itself, and for a trajectory that is not finished), D_w (n, N) the float64 against long double difference of
    the weights, window (n,) the least distance of a compared e to a window edge (form "window"; else inf)"""
    narrow = classify(form, potential, state, mass, window, gamma)
    wide_state = widen(state)
    wide = classify(form, potential, wide_state, mass, window, gamma)
    n = len(state[0])
    edge = np.full(n, np.inf)
    if AXES[axis]:
        edge = np.where(narrow["finished"], edge_distance(wide["energy"], grid).astype(np.float64), np.inf)
    near = np.full(n, np.inf)
    if form == "window":
        near = np.where(narrow["finished"], HQ.margin(HQ.energies(potential, wide_state)[0], window, gamma), np.inf)
    return dict(edge=edge, D_w=np.abs(narrow["w"] - wide["w"]).astype(np.float64), window=near)


class _OutgoingCalls:
    """the three calls on the restatement and the adiabatic energies hopping.outgoing_grids sizes its grids with; every call is recorded"""

    def pes_adiabatic_n(self, num_pes, model, x):
        self.calls.append(("adiabatic",))
        _, E, _, F = HN.states(np.asarray(x, dtype=np.float64), self._potential(num_pes, model))
        return E, F

    def hop_outgoing(self, num_pes, model, state, mass, grid, axis="momentum", acc=None):
        self.calls.append(("outgoing", axis))
        return outgoing("surface", self._potential(num_pes, model), state, mass, grid, axis, acc=acc)

    def hop_outgoing_mf(self, num_pes, model, state, mass, grid, axis="momentum", acc=None):
        self.calls.append(("outgoing_mf", axis))
        return outgoing("amplitude", self._potential(num_pes, model), state, mass, grid, axis, acc=acc)

    def hop_outgoing_sqc(self, num_pes, model, state, mass, grid, axis="momentum", window=HQ.TRIANGLE, gamma=None, acc=None):
        self.calls.append(("outgoing_sqc", axis, window, gamma))
        return outgoing("window", self._potential(num_pes, model), state, mass, grid, axis, window, HQ.GAMMA[window] if gamma is None else gamma, acc=acc)


class NumpyOutgoingApi(_OutgoingCalls, HS.NumpyScanApi):
    pass


class NumpyMfOutgoingApi(_OutgoingCalls, HM.NumpyMfApi):
    pass


class NumpySqcOutgoingApi(_OutgoingCalls, HQ.NumpySqcApi):
    pass


class NumpyMashOutgoingApi(_OutgoingCalls, HA.NumpyMashApi):
    pass


APIS = {"fssh": NumpyOutgoingApi, "ehrenfest": NumpyMfOutgoingApi, "sqc": NumpySqcOutgoingApi, "mash": NumpyMashOutgoingApi}
FORM_OF = {"fssh": "surface", "ehrenfest": "amplitude", "sqc": "window", "mash": "surface"}
