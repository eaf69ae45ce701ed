"""numpy restatement of the Ehrenfest (mean-field) trajectories of csrc/gple_hop.hip (gple_hop_evolve_mf / _observe_mf and their _groups forms;
include/gple.h, DESIGN.md §17, "Mean-field (Ehrenfest) trajectories"), written from the step as the header states it on top of
tests/hop_numpy.py's builtin, table, jacobi and states; vectorised over trajectories and generic in dtype (float64 and numpy.longdouble).

    force()                              b^dagger Fd b in the header's order
    evolve(), observe_terms(), observe() the entry points; evolve also returns per-trajectory diagnostics
    evolve_groups(), observe_groups()    every group is the plain call on its slice with the group's time step
    NumpyMfApi                           the four Api methods on this restatement (beside the sample and the FSSH ones), for hopping.run / scan
"""
import numpy as np

from tests import hop_numpy as HN
from tests import hop_scan_numpy as HS


def norms(b):
    return b.real * b.real + b.imag * b.imag


def force(Fd, b):
    """f = sum_i |b_i|^2 Fd_ii + 2 sum_{i<j} Fd_ij Re(conj(b_i) b_j): one running sum, the diagonal with i ascending, then the pairs ascending"""
    N = b.shape[1]
    f = np.zeros(b.shape[0], dtype=Fd.dtype)
    for i in range(N):
        f = f + norms(b[:, i]) * Fd[:, i, i]
    for i in range(N):
        for j in range(i + 1, N):
            f = f + 2.0 * Fd[:, i, j] * (b[:, i].real * b[:, j].real + b[:, i].imag * b[:, j].imag)
    return f


def energy(V, p, b, mass):
    """p^2 / 2m + b^dagger V b, which is p^2 / 2m + sum_k |c_k|^2 E_k in the diabatic representation"""
    return p * p / 2.0 / mass + np.einsum("mi,mij,mj->m", np.conj(b), V, b).real


def evolve(potential, state, mass, dt, n_steps, x_left, x_right, flip=False):
    """gple_hop_evolve_mf on a copy of the ensemble, in the dtype of its x -> (state, diagnostics).  surface is handed through.  Per trajectory:
    edge = the least |x_new - bound| over its steps and both bounds, drift = the largest |energy after a step - energy at the start| (float64).
    flip: every eigenvector of the mid-point matrix with the other sign"""
    x, p, b, surface, status = state
    x, p, b, status = (np.array(a) for a in (x, p, b, status))
    dtype, n = x.dtype, len(x)
    ty = dtype.type
    mass, dt, x_left, x_right = ty(mass), ty(dt), ty(x_left), ty(x_right)
    diag = dict(edge=np.full(n, np.inf), drift=np.zeros(n))
    live = np.nonzero(status == 0)[0]
    if len(live) == 0 or n_steps == 0:
        return (x, p, b, surface, status), diag
    Vx, Fx = potential(x[live])
    e0 = energy(Vx, p[live], b[live], mass)
    for _ in range(n_steps):
        xs, ps, bs = x[live], p[live], b[live]
        # 1
        ps = ps + force(Fx, bs) * dt / 2.0
        xn = xs + ps / mass * dt
        # 2
        Vn, Fn = potential(xn)
        lam, W = HN.jacobi(0.5 * (Vx + Vn))
        if flip:
            W = -W
        angle = lam * dt
        U = np.einsum("mik,mk,mjk->mij", W, np.cos(angle) - 1j * np.sin(angle), W)
        bs = np.einsum("mij,mj->mi", U, bs)
        # 3
        ps = ps + force(Fn, bs) * dt / 2.0
        # 4
        diag["edge"][live] = np.minimum(diag["edge"][live], np.minimum(np.abs(xn - x_left), np.abs(xn - x_right)).astype(np.float64))
        diag["drift"][live] = np.maximum(diag["drift"][live], np.abs(energy(Vn, ps, bs, mass) - e0).astype(np.float64))
        out = np.where(xn < x_left, 1, np.where(xn > x_right, 2, 0))
        x[live], p[live], b[live], status[live] = xn, ps, bs, out
        keep = out == 0
        live, Vx, Fx, e0 = live[keep], Vn[keep], Fn[keep], e0[keep]
        if len(live) == 0:
            break
    return (x, p, b, surface, status), diag


def observe_terms(potential, state, mass):
    """the (n, 3 N + 6) terms gple_hop_observe_mf sums, in its order; a status out of range adds to no weight and to no count"""
    x, p, b, _, status = state
    N, n = b.shape[1], len(x)
    status = np.asarray(status)
    _, E, C, _ = HN.states(x, potential)
    c = np.einsum("mik,mi->mk", C, b)
    w = norms(c)
    terms = np.zeros((n, 3 * N + 6), dtype=x.dtype)
    potential_energy = np.zeros(n, dtype=x.dtype)
    for k in range(N):
        potential_energy = potential_energy + w[:, k] * E[:, k]
    for s in range(3):
        terms[:, s * N:(s + 1) * N] = np.where((status == s)[:, None], w, 0)
        terms[:, 3 * N + s] = status == s
    terms[:, 3 * N + 3], terms[:, 3 * N + 4] = x, p
    terms[:, 3 * N + 5] = p * p / 2.0 / x.dtype.type(mass) + potential_energy
    return terms


def observe(potential, state, mass):
    return observe_terms(potential, state, mass).sum(axis=0)


def evolve_groups(potential, state, n_per_group, mass, dt, n_steps, x_left, x_right):
    """gple_hop_evolve_groups_mf on a copy -> (state, diagnostics): group g is evolve() on its slice with dt[g]"""
    n = len(state[0])
    n_groups = n // n_per_group
    assert n_groups * n_per_group == n and len(dt) == n_groups
    parts, diags = [], []
    for g, sl in enumerate(HS.slices(n_groups, n_per_group)):
        part, diag = evolve(potential, tuple(a[sl] for a in state), mass, dt[g], n_steps, x_left, x_right)
        parts.append(part)
        diags.append(diag)
    out = tuple(state[3] if q == 3 else np.concatenate([part[q] for part in parts]) for q in range(5))
    return out, {key: np.concatenate([d[key] for d in diags]) for key in diags[0]}


def observe_groups(potential, state, n_per_group, mass):
    """gple_hop_observe_groups_mf -> (n_groups, 3 N + 6): row g is observe() on the slice"""
    n_groups = len(state[0]) // n_per_group
    return np.stack([observe(potential, tuple(a[sl] for a in state), mass) for sl in HS.slices(n_groups, n_per_group)])


class NumpyMfApi(HS.NumpyScanApi):
    """Api.hop_evolve_mf / hop_observe_mf / hop_evolve_groups_mf / hop_observe_groups_mf on the restatement, beside the samples and the FSSH
    methods of NumpyScanApi; every call is recorded in `calls`"""

    def hop_evolve_mf(self, num_pes, model, state, mass, dt, n_steps, x_left, x_right):
        self.calls.append(("evolve_mf", n_steps))
        return evolve(self._potential(num_pes, model), state, mass, dt, n_steps, x_left, x_right)[0]

    def hop_observe_mf(self, num_pes, model, state, mass):
        self.calls.append(("observe_mf",))
        return observe(self._potential(num_pes, model), state, mass).astype(np.float64)

    def hop_evolve_groups_mf(self, num_pes, model, state, n_per_group, mass, dt, n_steps, x_left, x_right):
        self.calls.append(("evolve_groups_mf", n_steps))
        return evolve_groups(self._potential(num_pes, model), state, n_per_group, mass, dt, n_steps, x_left, x_right)[0]

    def hop_observe_groups_mf(self, num_pes, model, state, n_per_group, mass):
        self.calls.append(("observe_groups_mf",))
        return observe_groups(self._potential(num_pes, model), state, n_per_group, mass).astype(np.float64)
