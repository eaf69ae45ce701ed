"""numpy restatement of the MASH trajectories of csrc/gple_hop.hip (gple_hop_sample_mash / _evolve_mash and their _groups forms; include/gple.h,
DESIGN.md §17, "MASH trajectories"; Mannouch and Richardson, J. Chem. Phys. 158, 104111 (2023)), written from the definition as the header states
it, operation for operation, on top of tests/hop_numpy.py (potentials, jacobi, states, the Philox uniforms) and tests/hop_scan_numpy.py (the
grouped sample); vectorised over trajectories and generic in dtype (float64 and numpy.longdouble).  Two levels only.

    side()                                  1 where |c_1|^2 > |c_0|^2 else 0
    spin(), sample(), sample_groups()       s = |S_z| and the angle of a draw; the samples: x, p, surface and status are hop_numpy.sample's
    evolve()                                the step, with per-trajectory diagnostics and, on request, the history of every step
    evolve_groups()                         every group is the plain call on its slice, plus the counters of hops taken and frustrated
    NumpyMashApi                            the four Api methods on this restatement beside those of NumpyScanApi, for hopping.run / scan
The sums are hop_numpy.observe's: a MASH ensemble has the layout of a fewest-switches one.
"""
import numpy as np

from tests import hop_numpy as HN
from tests import hop_scan_numpy as HS


def norms(c):
    """|c_k|^2 = re re + im im"""
    return c.real * c.real + c.imag * c.imag


def side(c):
    """(n,) int64: 1 where |c_1|^2 > |c_0|^2 else 0, for c (n, 2)"""
    w = norms(c)
    return (w[:, 1] > w[:, 0]).astype(np.int64)


def adiabatic(C, b):
    """c = C^T b"""
    return np.einsum("mik,mi->mk", C, b)


def spin(index, seed, dtype=np.float64):
    """(s, w1) of the trajectories `index`: (w0, w1) = unit53 of the words (0, 1) and (2, 3) of the counter (index, 0, 3, 0), s = sqrt(1 - w0)"""
    ty = np.dtype(dtype).type
    w0, w1 = HN.uniforms(index, (0, 3, 0), seed)
    return np.sqrt(ty(1) - w0.astype(dtype)), w1.astype(dtype)


def _amplitudes(potential, x, index, seed, surface0):
    """b = C(x) c with c_a = sqrt((1 + s) / 2) and c_o = sqrt((1 - s) / 2) (cospi(2 w1) + i sinpi(2 w1)), a = surface0, o = 1 - a"""
    ty = x.dtype.type
    s, w1 = spin(index, seed, x.dtype)
    angle = (8.0 * np.arctan(ty(1))) * w1
    c = np.zeros((len(x), 2), dtype=HN.complex_of(x.dtype))
    c[:, surface0] = np.sqrt((ty(1) + s) / ty(2))
    c[:, 1 - surface0] = np.sqrt((ty(1) - s) / ty(2)) * (np.cos(angle) + 1j * np.sin(angle))
    _, _, C, _ = HN.states(x, potential)
    return np.einsum("mik,mk->mi", C, c).astype(HN.complex_of(x.dtype))


def _two_levels(num_pes):
    if num_pes != 2:
        raise ValueError("MASH is a two-level method")


def sample(potential, num_pes, n, seed, x0, p0, sigma_x, sigma_p, surface0=0, trajectory_offset=0, dtype=np.float64):
    """gple_hop_sample_mash -> (x, p, b, surface, status): x, p, surface and status are hop_numpy.sample's"""
    _two_levels(num_pes)
    x, p, _, surface, status = HN.sample(potential, num_pes, n, seed, x0, p0, sigma_x, sigma_p, surface0, trajectory_offset, dtype)
    return x, p, _amplitudes(potential, x, trajectory_offset + np.arange(n), seed, surface0), surface, status


def sample_groups(potential, num_pes, n_per_group, seed, packets, surface0=0, trajectory_offset=0, dtype=np.float64):
    """gple_hop_sample_groups_mash: x, p, surface and status are hop_scan_numpy.sample_groups's (the zero-sigma select included)"""
    _two_levels(num_pes)
    x, p, _, surface, status = HS.sample_groups(potential, num_pes, n_per_group, seed, packets, surface0, trajectory_offset, dtype)
    return x, p, _amplitudes(potential, x, trajectory_offset + np.arange(len(x)), seed, surface0), surface, status


def evolve(potential, state, mass, dt, n_steps, x_left, x_right, flip=False, history=False):
    """gple_hop_evolve_mash on a copy of the ensemble, in the dtype of its x -> (state, diagnostics).  Per trajectory: hops, frustrated (counts),
    margin = the least | |c_1|^2 - |c_0|^2 | over the start point and its steps, ratio = the least |r| / p^2 where a hop was attempted, edge = the
    least |x_new - bound| for either bound (inf where there was none).  flip: every eigenvector with the other sign.  history: diag["steps"] is a
    list with one dict per step of arrays over the trajectories that took it: index, a_before, a, side_old, side, p_before (after the second
    half kick), p, taken, stuck, E_before = p_before^2 / 2m + E_a_before, E_after = p^2 / 2m + E_a, norm = sum_k |b_k|^2"""
    x, p, b, surface, status = (np.array(a) for a in state)
    _two_levels(b.shape[1])
    dtype, n = x.dtype, len(x)
    ty = dtype.type
    mass, dt, x_left, x_right = ty(mass), ty(dt), ty(x_left), ty(x_right)
    diag = dict(hops=np.zeros(n, dtype=np.int64), frustrated=np.zeros(n, dtype=np.int64), margin=np.full(n, np.inf), ratio=np.full(n, np.inf),
                edge=np.full(n, np.inf), steps=[] if history else None)
    live = np.nonzero(status == 0)[0]
    if len(live) == 0 or n_steps == 0:
        return (x, p, b, surface, status), diag

    def side_of(C, bs, who):
        c = adiabatic(C, bs)
        w = norms(c)
        diag["margin"][who] = np.minimum(diag["margin"][who], np.abs(w[:, 1] - w[:, 0]).astype(np.float64))
        return side(c)

    # the pass s = -1: the states and the side at the start point
    Vx, _, Cx, Fx = HN.states(x[live], potential, flip)
    side_old = side_of(Cx, b[live], live)
    for _ in range(n_steps):
        xs, ps, bs, a = x[live], p[live], b[live], surface[live].astype(np.int64)
        row = np.arange(len(live))
        # 1
        ps = ps + Fx[row, a, a] * dt / 2.0
        xn = xs + ps / mass * dt
        # 2
        Vn, E, C, F = HN.states(xn, potential, flip)
        lam, W = HN.jacobi(0.5 * (Vx + Vn))
        if flip:
            W = -W
        angle = lam * dt
        U = np.einsum("mik,mk,mjk->mij", W, np.cos(angle) - 1j * np.sin(angle), W)
        bs = np.einsum("mij,mj->mi", U, bs)
        # 3
        ps = ps + F[row, a, a] * dt / 2.0
        # 4
        side_new = side_of(C, bs, live)
        # 5
        cross = (side_new != side_old) & (side_new != a)
        Ea = E[row, a]
        r = ps * ps + 2.0 * mass * (Ea - E[row, side_new])
        jump, stuck = cross & (r >= 0), cross & (r < 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            diag["ratio"][live] = np.minimum(diag["ratio"][live], np.where(cross, np.abs(r) / (ps * ps), np.inf).astype(np.float64))
        before = ps
        ps = np.where(jump, np.sign(ps) * np.sqrt(np.where(jump, r, ty(0))), ps)
        ps = np.where(stuck, -ps, ps)
        a_new = np.where(jump, side_new, a)
        diag["hops"][live] += jump
        diag["frustrated"][live] += stuck
        if history:
            diag["steps"].append(dict(index=live.copy(), a_before=a, a=a_new, side_old=side_old, side=side_new, p_before=before, p=ps, taken=jump, stuck=stuck,
                                      E_before=before * before / 2.0 / mass + Ea, E_after=ps * ps / 2.0 / mass + E[row, a_new], norm=norms(bs).sum(axis=1)))
        # 6
        diag["edge"][live] = np.minimum(diag["edge"][live], np.minimum(np.abs(xn - x_left), np.abs(xn - x_right)).astype(np.float64))
        out = np.where(xn < x_left, 1, np.where(xn > x_right, 2, 0))
        x[live], p[live], b[live], surface[live], status[live] = xn, ps, bs, a_new, out
        keep = out == 0
        live, Vx, Fx, side_old = live[keep], Vn[keep], F[keep], side_new[keep]
        if len(live) == 0:
            break
    return (x, p, b, surface, status), diag


def set_aside(diag):
    """the trajectories whose float64 decisions are within rounding: the least side margin below 1e-10, or an attempted hop with |r| < 1e-9 p^2"""
    return (diag["margin"] < 1e-10) | (diag["ratio"] < 1e-9)


def evolve_groups(potential, state, n_per_group, mass, dt, n_steps, x_left, x_right, hops=None):
    """gple_hop_evolve_groups_mash on a copy -> (state, hops, diagnostics): group g is evolve() on its slice with dt[g]; hops (n, 2) int32 is a
    copy of the given counters (zeros for None) with the hops taken and the frustrated hops of the call added"""
    n = len(state[0])
    n_groups = n // n_per_group
    assert n_groups * n_per_group == n and len(dt) == n_groups
    hops = np.zeros((n, 2), dtype=np.int32) if hops is None else np.array(hops, dtype=np.int32)
    parts, diags = [], []
    for g, sl in enumerate(HS.slices(n_groups, n_per_group)):
        part, diag = evolve(potential, tuple(a[sl] for a in state), mass, dt[g], n_steps, x_left, x_right)
        parts.append(part)
        diags.append(diag)
        hops[sl, 0] += diag["hops"].astype(np.int32)
        hops[sl, 1] += diag["frustrated"].astype(np.int32)
    out = tuple(np.concatenate([part[q] for part in parts]) for q in range(5))
    return out, hops, {key: np.concatenate([d[key] for d in diags]) for key in ("hops", "frustrated", "margin", "ratio", "edge")}


class NumpyMashApi(HS.NumpyScanApi):
    """Api.hop_sample_mash / hop_evolve_mash and their _groups forms on the restatement, beside the methods of NumpyScanApi (hop_observe and
    hop_observe_groups serve a MASH ensemble unchanged); every call is recorded in `calls`"""

    def hop_sample_mash(self, num_pes, model, n, seed, x0, p0, sigma_x, sigma_p, surface0=0, trajectory_offset=0, device_out=False):
        self.calls.append(("sample_mash", n))
        return sample(self._potential(num_pes, model), num_pes, n, seed, x0, p0, sigma_x, sigma_p, surface0, trajectory_offset, self.dtype)

    def hop_sample_groups_mash(self, num_pes, model, n_per_group, seed, packets, surface0=0, trajectory_offset=0, device_out=False):
        self.calls.append(("sample_groups_mash", len(packets), n_per_group))
        return sample_groups(self._potential(num_pes, model), num_pes, n_per_group, seed, packets, surface0, trajectory_offset, self.dtype)

    def hop_evolve_mash(self, num_pes, model, state, mass, dt, n_steps, x_left, x_right):
        self.calls.append(("evolve_mash", n_steps))
        return evolve(self._potential(num_pes, model), state, mass, dt, n_steps, x_left, x_right)[0]

    def hop_evolve_groups_mash(self, num_pes, model, state, n_per_group, mass, dt, n_steps, x_left, x_right, hops=None):
        self.calls.append(("evolve_groups_mash", n_steps))
        out, counted, _ = evolve_groups(self._potential(num_pes, model), state, n_per_group, mass, dt, n_steps, x_left, x_right, hops)
        return out if hops is None else (out, counted)
