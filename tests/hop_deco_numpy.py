"""numpy restatement of the surface hopping step WITH the decoherence correction 6a (gple_hop_evolve_dc / gple_hop_evolve_groups_dc; include/gple.h,
DESIGN.md §17, "Decoherence corrections"), written from the definition in the header.  tests/hop_numpy.py is not edited: its step is restated
here in full with the stage between steps 6 and 7, on its own states, jacobi, uniforms and potentials, vectorised over trajectories and generic
in dtype (float64 and numpy.longdouble).  With mode NONE the operations are hop_numpy.evolve's, one for one: the same bits.

    stage()                     step 6a alone, on the adiabatic amplitudes
    evolve(), evolve_groups()   gple_hop_evolve_dc, gple_hop_evolve_groups_dc; the diagnostics of hop_numpy.evolve
    NumpyDecoApi                hop_evolve / hop_evolve_groups with the keywords decoherence and edc_c, beside everything NumpyScanApi has
"""
import numpy as np

from tests import hop_numpy as HN
from tests import hop_scan_numpy as HS

NONE, EDC, COLLAPSE_HOP, COLLAPSE_ATTEMPT = range(4)  # GPLE_HOP_DC_*
MODES = {None: NONE, "none": NONE, "edc": EDC, "collapse_hop": COLLAPSE_HOP, "collapse_attempt": COLLAPSE_ATTEMPT}
EDC_C = 0.1  # Hartree, the papers' value


def mode_of(decoherence):
    mode = MODES[decoherence] if decoherence in MODES else int(decoherence)
    if mode not in (NONE, EDC, COLLAPSE_HOP, COLLAPSE_ATTEMPT):
        raise ValueError(decoherence)
    return mode


def stage(c, E, a, p, mass, dt, mode, edc_c=EDC_C, wanted=None, taken=None):
    """Step 6a on c (m, N) complex, the adiabatic amplitudes of step 4, with the energies E (m, N), the active surface a and the momentum p AFTER
    step 6; wanted, taken (m,) bool: a hop was wanted at step 5, and taken at step 6.  -> (c, changed): a copy, and the rows 6a acted on (for
    which the caller sets b <- C c).  Real and imaginary parts are treated one by one, as the device does: no complex division"""
    c = np.array(c)
    m, N = c.shape
    ty = E.dtype.type
    row = np.arange(m)
    if mode == NONE:
        return c, np.zeros(m, dtype=bool)
    re, im = c.real.copy(), c.imag.copy()
    are, aim = re[row, a], im[row, a]
    na = are * are + aim * aim
    on = na != 0  # |c_a|^2 == 0 skips the stage
    safe = np.where(on, na, ty(1))
    if mode == EDC:
        kinetic = p * p / 2.0 / ty(mass)
        with np.errstate(divide="ignore", invalid="ignore"):
            w = np.ones(m, dtype=E.dtype) if edc_c == 0 else kinetic / (kinetic + ty(edc_c))
        Ea = E[row, a]
        lost = np.zeros(m, dtype=E.dtype)
        for k in range(N):
            other = on & (a != k)
            f = np.exp(-ty(dt) * np.abs(E[:, k] - Ea) * w)  # hbar = 1
            lost = lost + np.where(other, (re[:, k] * re[:, k] + im[:, k] * im[:, k]) * (1.0 - f * f), ty(0))
            re[:, k], im[:, k] = np.where(other, f * re[:, k], re[:, k]), np.where(other, f * im[:, k], im[:, k])
        grow = np.sqrt(1.0 + lost / safe)
        re[row, a], im[row, a] = np.where(on, are * grow, are), np.where(on, aim * grow, aim)
        changed = on
    else:
        changed = on & np.asarray(wanted if mode == COLLAPSE_ATTEMPT else taken, dtype=bool)
        length = np.sqrt(safe)
        re, im = np.where(changed[:, None], ty(0), re), np.where(changed[:, None], ty(0), im)
        re[row, a], im[row, a] = np.where(changed, are / length, are), np.where(changed, aim / length, aim)
    out = np.empty_like(c)
    out.real, out.imag = re, im
    return out, changed


def evolve(potential, state, seed, mass, dt, first_step, n_steps, x_left, x_right, reverse=False, trajectory_offset=0, flip=False, decoherence=None,
           edc_c=EDC_C):
    """gple_hop_evolve_dc on a copy of the ensemble, in the dtype of its x -> (state, diagnostics), the diagnostics being hop_numpy.evolve's: per
    trajectory hops, frustrated (counts), margin, ratio, edge.  flip: every eigenvector with the other sign"""
    mode = mode_of(decoherence)
    x, p, b, surface, status = (np.array(a) for a in state)
    dtype, n = x.dtype, len(x)
    ty = dtype.type
    mass, dt, x_left, x_right = ty(mass), ty(dt), ty(x_left), ty(x_right)
    diag = dict(hops=np.zeros(n, dtype=np.int64), frustrated=np.zeros(n, dtype=np.int64), margin=np.full(n, np.inf), ratio=np.full(n, np.inf),
                edge=np.full(n, np.inf))
    live = np.nonzero(status == 0)[0]
    if len(live) == 0 or n_steps == 0:
        return (x, p, b, surface, status), diag
    N = b.shape[1]
    Vx, _, _, Fx = HN.states(x[live], potential, flip)
    for s in range(n_steps):
        step = first_step + s
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
        c = np.einsum("mik,mi->mk", C, bs)
        ca, Ea = c[row, a], E[row, a]
        na = ca.real * ca.real + ca.imag * ca.imag
        v = ps / mass
        g = np.zeros((len(live), N), dtype=dtype)
        for k in range(N):
            Fak = F[row, a, k]
            on = (a != k) & (na != 0) & (Fak != 0)
            with np.errstate(divide="ignore", invalid="ignore"):
                d = Fak / np.where(on, Ea - E[:, k], ty(1))
                gk = np.fmax(ty(0), 2.0 * dt * v * d * (ca.real * c[:, k].real + ca.imag * c[:, k].imag) / np.where(on, na, ty(1)))
            g[:, k] = np.where(on, gk, ty(0))
        # 5
        xi, _ = HN.uniforms(trajectory_offset + live, (step & 0xFFFFFFFF, 0, step >> 32), seed)
        xi = xi.astype(dtype)
        cum = np.cumsum(g, axis=1)  # g_a = 0: the sum over k != a in ascending order
        other = a[:, None] != np.arange(N)[None, :]
        wanted = other & (xi[:, None] < cum)
        hop = wanted.any(axis=1)
        target = np.where(hop, np.argmax(wanted, axis=1), a)
        diag["margin"][live] = np.minimum(diag["margin"][live], np.min(np.where(other, np.abs(xi[:, None] - cum), np.inf), axis=1).astype(np.float64))
        # 6
        r = ps * ps + 2.0 * mass * (Ea - E[row, target])
        jump, stuck = hop & (r >= 0), hop & (r < 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            diag["ratio"][live] = np.minimum(diag["ratio"][live], np.where(hop, np.abs(r) / (ps * ps), np.inf).astype(np.float64))
        ps = np.where(jump, np.sign(ps) * np.sqrt(np.where(jump, r, ty(0))), ps)
        if reverse:
            ps = np.where(stuck, -ps, ps)
        a = np.where(jump, target, a)
        diag["hops"][live] += jump
        diag["frustrated"][live] += stuck
        # 6a: on the c of step 4, with a and p as step 6 left them; b <- C c where it acted
        if mode != NONE:
            c, changed = stage(c, E, a, ps, mass, dt, mode, edc_c, wanted=hop, taken=jump)
            bs = np.where(changed[:, None], np.einsum("mik,mk->mi", C, c), bs)
        # 7
        diag["edge"][live] = np.minimum(diag["edge"][live], np.minimum(np.abs(xn - x_left), np.abs(xn - x_right)).astype(np.float64))
        out = np.where(xn < x_left, 1, np.where(xn > x_right, 2, 0))
        x[live], p[live], b[live], surface[live], status[live] = xn, ps, bs, a, out
        keep = out == 0
        live, Vx, Fx = live[keep], Vn[keep], F[keep]
        if len(live) == 0:
            break
    return (x, p, b, surface, status), diag


def evolve_groups(potential, state, n_per_group, seed, mass, dt, first_step, n_steps, x_left, x_right, reverse=False, trajectory_offset=0, hops=None,
                  decoherence=None, edc_c=EDC_C):
    """gple_hop_evolve_groups_dc on a copy -> (state, hops, diagnostics), as hop_scan_numpy.evolve_groups: group g is evolve() on its slice with
    dt[g] and the group's offset (neighbours with the same time step share one call: trajectories are independent)"""
    n = len(state[0])
    n_groups = n // n_per_group
    assert n_groups * n_per_group == n and len(dt) == n_groups
    hops = np.zeros((n, 2), dtype=np.int32) if hops is None else np.array(hops, dtype=np.int32)
    parts, diags, g = [], [], 0
    sl = HS.slices(n_groups, n_per_group)
    while g < n_groups:
        last = g
        while last + 1 < n_groups and dt[last + 1] == dt[g]:
            last += 1
        span = slice(sl[g].start, sl[last].stop)
        part, diag = evolve(potential, tuple(a[span] for a in state), seed, mass, dt[g], first_step, n_steps, x_left, x_right, reverse,
                            trajectory_offset + g * n_per_group, decoherence=decoherence, edc_c=edc_c)
        parts.append(part)
        diags.append(diag)
        hops[span, 0] += diag["hops"].astype(np.int32)
        hops[span, 1] += diag["frustrated"].astype(np.int32)
        g = last + 1
    out = tuple(np.concatenate([part[q] for part in parts]) for q in range(5))
    return out, hops, {key: np.concatenate([d[key] for d in diags]) for key in diags[0]}


class NumpyDecoApi(HS.NumpyScanApi):
    """Api.hop_evolve / hop_evolve_groups with the keywords decoherence and edc_c on this restatement; `calls` holds what NumpyScanApi records,
    `keywords` the (decoherence, edc_c) of every evolve call, in order"""

    def __init__(self, potentials=None, dtype=np.float64):
        super().__init__(potentials, dtype)
        self.keywords = []

    def hop_evolve(self, num_pes, model, state, seed, mass, dt, first_step, n_steps, x_left, x_right, reverse=False, trajectory_offset=0, decoherence=None,
                   edc_c=EDC_C):
        self.calls.append(("evolve", first_step, n_steps))
        self.keywords.append((decoherence, edc_c))
        return evolve(self._potential(num_pes, model), state, seed, mass, dt, first_step, n_steps, x_left, x_right, reverse, trajectory_offset,
                      decoherence=decoherence, edc_c=edc_c)[0]

    def hop_evolve_groups(self, num_pes, model, state, n_per_group, seed, mass, dt, first_step, n_steps, x_left, x_right, reverse=False, trajectory_offset=0,
                          hops=None, decoherence=None, edc_c=EDC_C):
        self.calls.append(("evolve_groups", first_step, n_steps))
        self.keywords.append((decoherence, edc_c))
        out, counted, _ = evolve_groups(self._potential(num_pes, model), state, n_per_group, seed, mass, dt, first_step, n_steps, x_left, x_right, reverse,
                                        trajectory_offset, hops, decoherence=decoherence, edc_c=edc_c)
        return out if hops is None else (out, counted)
