"""numpy restatement of the symmetrical quasi-classical trajectories of csrc/gple_hop.hip (gple_hop_sample_sqc / _evolve_sqc / _observe_sqc and their
_groups forms; include/gple.h, DESIGN.md §17, "Symmetrical quasi-classical trajectories"), written from the definitions as the header states them on
top of tests/hop_numpy.py (potentials, jacobi, states, the Philox uniforms) and tests/hop_mf_numpy.py (the mean-field running sum); vectorised
over trajectories and generic in dtype (float64 and numpy.longdouble).

    start_energies(), sample()             the start windows; x and p are hop_numpy.sample's
    force(), hamiltonian(), evolve()       the step (the mean-field one with f = b^dagger Fd b - gamma tr Fd) with per-trajectory diagnostics
    energies(), window_of(), margin()      e = |C^T b|^2, the final window of every trajectory (-1: none), the distance of e to the window edges
    observe_terms(), observe()             the 4 N + 9 terms and their sums
    sample_groups(), evolve_groups(), observe_groups()   every group is the plain call on its slice
    NumpySqcApi                            the six Api methods on this restatement, for hopping.run / scan; every call is recorded
"""
import numpy as np

from tests import hop_mf_numpy as HM
from tests import hop_numpy as HN
from tests import hop_scan_numpy as HS

SQUARE, TRIANGLE = 0, 1
GAMMA = {SQUARE: (np.sqrt(3.0) - 1.0) / 2.0, TRIANGLE: 1.0 / 3.0}


def start_energies(u, surface0, window, gamma):
    """e (n, N) on the start window of state surface0 from the uniforms u (n, N), in u's dtype"""
    n, N = u.shape
    ty = u.dtype.type
    occupied = np.arange(N) == surface0
    if window == SQUARE:
        return np.where(occupied[None, :], ty(1), ty(0)) + ty(2.0) * ty(gamma) * u
    root = ty(1) - u[:, surface0]
    t = np.sqrt(root) if N == 2 else np.cbrt(root)
    return np.where(occupied[None, :], (ty(2) - t)[:, None], u * t[:, None])


def _amplitudes(potential, x, e, v):
    """b = C(x) c with c_k = sqrt(e_k) (cospi(2 v_k) + i sinpi(2 v_k))"""
    ty = x.dtype.type
    angle = (8.0 * np.arctan(ty(1))) * v
    c = np.sqrt(e) * (np.cos(angle) + 1j * np.sin(angle))
    _, _, C, _ = HN.states(x, potential)
    return np.einsum("mik,mk->mi", C, c).astype(HN.complex_of(x.dtype))


def level_uniforms(index, num_pes, seed, dtype):
    """(u, v) (n, N): level k draws unit53 of the words (0, 1) and (2, 3) of the counter (index, k, 2, 0)"""
    pairs = [HN.uniforms(index, (k, 2, 0), seed) for k in range(num_pes)]
    return np.stack([q[0] for q in pairs], axis=1).astype(dtype), np.stack([q[1] for q in pairs], axis=1).astype(dtype)


def sample(potential, num_pes, n, seed, x0, p0, sigma_x, sigma_p, surface0=0, window=TRIANGLE, gamma=None, trajectory_offset=0, dtype=np.float64):
    """gple_hop_sample_sqc -> (x, p, b, surface, status): x, p, surface and status are hop_numpy.sample's"""
    gamma = GAMMA[window] if gamma is None else gamma
    x, p, _, surface, status = HN.sample(potential, num_pes, n, seed, x0, p0, sigma_x, sigma_p, surface0, trajectory_offset, dtype)
    u, v = level_uniforms(trajectory_offset + np.arange(n), num_pes, seed, dtype)
    return x, p, _amplitudes(potential, x, start_energies(u, surface0, window, gamma), v), surface, status


def sample_groups(potential, num_pes, n_per_group, seed, packets, surface0=0, window=TRIANGLE, gamma=None, trajectory_offset=0, dtype=np.float64):
    """gple_hop_sample_groups_sqc: x, p, surface and status are hop_scan_numpy.sample_groups's (the zero-sigma select included)"""
    gamma = GAMMA[window] if gamma is None else gamma
    x, p, _, surface, status = HS.sample_groups(potential, num_pes, n_per_group, seed, packets, surface0, trajectory_offset, dtype)
    u, v = level_uniforms(trajectory_offset + np.arange(len(x)), num_pes, seed, dtype)
    return x, p, _amplitudes(potential, x, start_energies(u, surface0, window, gamma), v), surface, status


def trace(A):
    """the diagonal added left to right"""
    t = A[:, 0, 0]
    for i in range(1, A.shape[1]):
        t = t + A[:, i, i]
    return t


def force(Fd, b, gamma):
    """the mean-field running sum, then minus gamma times the trace"""
    return HM.force(Fd, b) - Fd.dtype.type(gamma) * trace(Fd)


def hamiltonian(V, p, b, mass, gamma):
    """p^2 / 2m + b^dagger V b - gamma tr V"""
    return HM.energy(V, p, b, mass) - V.dtype.type(gamma) * trace(V)


def evolve(potential, state, mass, dt, n_steps, x_left, x_right, gamma, flip=False, drift=True):
    """gple_hop_evolve_sqc on a copy of the ensemble, in the dtype of its x -> (state, diagnostics).  surface is handed through.  Per
    trajectory: edge = the least |x_new - bound| over its steps and both bounds, drift = the largest |H after a step - H at the start|.
    flip: every eigenvector of the mid-point matrix with the other sign; drift=False leaves that diagnostic out (it costs a third of the time)"""
    x, p, b, surface, status = state
    x, p, b, status = (np.array(a) for a in (x, p, b, status))
    dtype, n = x.dtype, len(x)
    ty = dtype.type
    mass, dt, x_left, x_right = ty(mass), ty(dt), ty(x_left), ty(x_right)
    diag = dict(edge=np.full(n, np.inf), drift=np.zeros(n) if drift else None)
    live = np.nonzero(status == 0)[0]
    if len(live) == 0 or n_steps == 0:
        return (x, p, b, surface, status), diag
    Vx, Fx = potential(x[live])
    h0 = hamiltonian(Vx, p[live], b[live], mass, gamma) if drift else np.zeros(len(live))
    for _ in range(n_steps):
        xs, ps, bs = x[live], p[live], b[live]
        ps = ps + force(Fx, bs, gamma) * dt / 2.0
        xn = xs + ps / mass * dt
        Vn, Fn = potential(xn)
        lam, W = HN.jacobi(0.5 * (Vx + Vn))
        if flip:
            W = -W
        angle = lam * dt
        U = np.einsum("mik,mk,mjk->mij", W, np.cos(angle) - 1j * np.sin(angle), W)
        bs = np.einsum("mij,mj->mi", U, bs)
        ps = ps + force(Fn, bs, gamma) * dt / 2.0
        diag["edge"][live] = np.minimum(diag["edge"][live], np.minimum(np.abs(xn - x_left), np.abs(xn - x_right)).astype(np.float64))
        if drift:
            diag["drift"][live] = np.maximum(diag["drift"][live], np.abs(hamiltonian(Vn, ps, bs, mass, gamma) - h0).astype(np.float64))
        out = np.where(xn < x_left, 1, np.where(xn > x_right, 2, 0))
        x[live], p[live], b[live], status[live] = xn, ps, bs, out
        keep = out == 0
        live, Vx, Fx, h0 = live[keep], Vn[keep], Fn[keep], h0[keep]
        if len(live) == 0:
            break
    return (x, p, b, surface, status), diag


def energies(potential, state):
    """(e (n, N) = |c_k|^2 with c = C^T b at the trajectory's x, E (n, N))"""
    x, _, b = state[:3]
    _, E, C, _ = HN.states(x, potential)
    return HM.norms(np.einsum("mik,mi->mk", C, b)), E


def _comparisons(e, window, gamma):
    """per state k (a list of N): the list of (left side, edge, sense) the window of k compares, sense +1: left >= edge, -1: left <= edge"""
    N = e.shape[1]
    ty = e.dtype.type
    out = []
    for k in range(N):
        if window == SQUARE:
            tests = [(e[:, k], ty(1), 1), (e[:, k], ty(1) + ty(2.0) * ty(gamma), -1)] + [(e[:, j], ty(2.0) * ty(gamma), -1) for j in range(N) if j != k]
        else:
            tests = [(e[:, k], ty(1), 1)] + [(e[:, k] + e[:, j], ty(2), -1) for j in range(N) if j != k]
        out.append(tests)
    return out


def window_of(e, window, gamma):
    """the first k ascending whose final window holds e, else -1"""
    found = np.full(len(e), -1, dtype=np.int64)
    for k, tests in reversed(list(enumerate(_comparisons(e, window, gamma)))):
        inside = np.ones(len(e), dtype=bool)
        for left, edge, sense in tests:
            inside &= (left >= edge) if sense > 0 else (left <= edge)
        found = np.where(inside, k, found)
    return found


def margin(e, window, gamma):
    """per trajectory the least distance of a compared quantity to the edge it is compared with, over every comparison of every window"""
    m = np.full(len(e), np.inf)
    for tests in _comparisons(e, window, gamma):
        for left, edge, _ in tests:
            m = np.minimum(m, np.abs(left - edge).astype(np.float64))
    return m


def observe_terms(potential, state, mass, window, gamma):
    """the (n, 4 N + 9) terms gple_hop_observe_sqc sums, in its order; a status out of range adds nowhere"""
    x, p, b, _, status = state
    N, n = b.shape[1], len(x)
    ty = x.dtype.type
    status = np.asarray(status)
    e, E = energies(potential, state)
    found = window_of(e, window, gamma)
    counted = (status >= 0) & (status <= 2)
    terms = np.zeros((n, 4 * N + 9), dtype=x.dtype)
    potential_energy = np.zeros(n, dtype=x.dtype)
    for k in range(N):
        potential_energy = potential_energy + (e[:, k] - ty(gamma)) * E[:, k]
    for s in range(3):
        for k in range(N):
            terms[:, s * N + k] = (status == s) & (found == k)
        terms[:, 3 * N + s] = status == s
        terms[:, 3 * N + 3 + s] = (status == s) & (found < 0)
    terms[:, 3 * N + 6:4 * N + 6] = np.where(counted[:, None], e, 0)
    terms[:, 4 * N + 6], terms[:, 4 * N + 7] = np.where(counted, x, 0), np.where(counted, p, 0)
    terms[:, 4 * N + 8] = np.where(counted, p * p / 2.0 / ty(mass) + potential_energy, 0)
    return terms


def observe(potential, state, mass, window, gamma):
    return observe_terms(potential, state, mass, window, gamma).sum(axis=0)


def evolve_groups(potential, state, n_per_group, mass, dt, n_steps, x_left, x_right, gamma):
    """gple_hop_evolve_groups_sqc on a copy -> (state, diagnostics): group g is evolve() on its slice with dt[g]"""
    n = len(state[0])
    n_groups = n // n_per_group
    assert n_groups * n_per_group == n and len(dt) == n_groups
    parts, diags = [], []
    for g, sl in enumerate(HS.slices(n_groups, n_per_group)):
        part, diag = evolve(potential, tuple(a[sl] for a in state), mass, dt[g], n_steps, x_left, x_right, gamma)
        parts.append(part)
        diags.append(diag)
    out = tuple(state[3] if q == 3 else np.concatenate([part[q] for part in parts]) for q in range(5))
    return out, {key: np.concatenate([d[key] for d in diags]) for key in diags[0]}


def observe_groups(potential, state, n_per_group, mass, window, gamma):
    """gple_hop_observe_groups_sqc -> (n_groups, 4 N + 9): row g is observe() on the slice"""
    n_groups = len(state[0]) // n_per_group
    return np.stack([observe(potential, tuple(a[sl] for a in state), mass, window, gamma) for sl in HS.slices(n_groups, n_per_group)])


class NumpySqcApi(HS.NumpyScanApi):
    """Api.hop_sample_sqc / hop_evolve_sqc / hop_observe_sqc and their _groups forms on the restatement, beside the methods of NumpyScanApi; every
    call is recorded in `calls`"""

    def hop_sample_sqc(self, num_pes, model, n, seed, x0, p0, sigma_x, sigma_p, surface0=0, window=TRIANGLE, gamma=None, trajectory_offset=0, device_out=False):
        self.calls.append(("sample_sqc", n, window, gamma))
        return sample(self._potential(num_pes, model), num_pes, n, seed, x0, p0, sigma_x, sigma_p, surface0, window, gamma, trajectory_offset, self.dtype)

    def hop_sample_groups_sqc(self, num_pes, model, n_per_group, seed, packets, surface0=0, window=TRIANGLE, gamma=None, trajectory_offset=0, device_out=False):
        self.calls.append(("sample_groups_sqc", len(packets), n_per_group, window, gamma))
        return sample_groups(self._potential(num_pes, model), num_pes, n_per_group, seed, packets, surface0, window, gamma, trajectory_offset, self.dtype)

    def hop_evolve_sqc(self, num_pes, model, state, mass, dt, n_steps, x_left, x_right, gamma):
        self.calls.append(("evolve_sqc", n_steps, gamma))
        return evolve(self._potential(num_pes, model), state, mass, dt, n_steps, x_left, x_right, gamma)[0]

    def hop_observe_sqc(self, num_pes, model, state, mass, window=TRIANGLE, gamma=None):
        self.calls.append(("observe_sqc", window, gamma))
        return observe(self._potential(num_pes, model), state, mass, window, GAMMA[window] if gamma is None else gamma).astype(np.float64)

    def hop_evolve_groups_sqc(self, num_pes, model, state, n_per_group, mass, dt, n_steps, x_left, x_right, gamma):
        self.calls.append(("evolve_groups_sqc", n_steps, gamma))
        return evolve_groups(self._potential(num_pes, model), state, n_per_group, mass, dt, n_steps, x_left, x_right, gamma)[0]

    def hop_observe_groups_sqc(self, num_pes, model, state, n_per_group, mass, window=TRIANGLE, gamma=None):
        self.calls.append(("observe_groups_sqc", window, gamma))
        return observe_groups(self._potential(num_pes, model), state, n_per_group, mass, window, GAMMA[window] if gamma is None else gamma).astype(np.float64)
