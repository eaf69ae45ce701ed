"""numpy restatement of the fewest-switches surface hopping of csrc/gple_hop.hip (include/gple.h), written from the step as the
header states it, vectorised over trajectories and generic in dtype: float64, and numpy.longdouble with its complex type (numpy.linalg.eigh has
no long double, hence the cyclic Jacobi below, which is the device's: 8 sweeps, a pair with an exactly zero entry not rotated, ascending order).

    builtin(model, num_pes), table(Table)   the diabatic potential as a function x -> (V, F = -V') in x's dtype
    sample(), evolve(), observe()           the three entry points; evolve also returns per-trajectory diagnostics
    NumpyHopApi                             the three Api methods on this restatement, for hopping.run
"""
import numpy as np

from oracle.evolve_oracle import philox4x32

SAC, DAC, ECR, TSAC = 0, 1, 2, 3
TWO53 = 9007199254740992.0


def _sgn(x):
    return (x > 0).astype(x.dtype) - (x < 0).astype(x.dtype)


def builtin(model, num_pes):
    """csrc/gple_pes_n.h, diabatic_n: the constants are the device's doubles, the arithmetic is x's dtype"""
    def fun(x):
        V, F = np.zeros(x.shape + (num_pes, num_pes), dtype=x.dtype), np.zeros(x.shape + (num_pes, num_pes), dtype=x.dtype)
        if model == SAC:
            e = np.exp(-_sgn(x) * 1.6 * x)
            V[:, 0, 0] = _sgn(x) * 0.01 * (1.0 - e)
            V[:, 1, 1] = -V[:, 0, 0]
            V[:, 0, 1] = V[:, 1, 0] = 0.005 * np.exp(-1.0 * x * x)
            F[:, 0, 0] = -0.01 * 1.6 * e
            F[:, 1, 1] = -F[:, 0, 0]
            F[:, 0, 1] = F[:, 1, 0] = 2.0 * 0.005 * 1.0 * x * np.exp(-1.0 * x * x)
        elif model == DAC:
            V[:, 1, 1] = 0.05 - 0.10 * np.exp(-0.28 * x * x)
            V[:, 0, 1] = V[:, 1, 0] = 0.015 * np.exp(-0.06 * x * x)
            F[:, 1, 1] = -2 * 0.10 * 0.28 * x * np.exp(-0.28 * x * x)
            F[:, 0, 1] = F[:, 1, 0] = 2 * 0.015 * 0.06 * x * np.exp(-0.06 * x * x)
        elif model == ECR:
            e = np.exp(-_sgn(x) * 0.90 * x)
            V[:, 0, 0], V[:, 1, 1] = 6e-4, -6e-4
            V[:, 0, 1] = V[:, 1, 0] = 0.10 * (1 - _sgn(x) * (e - 1))
            F[:, 0, 1] = F[:, 1, 0] = -0.10 * 0.90 * e
        elif model == TSAC and num_pes == 3:
            t, g, th = np.tanh(0.8 * x), 1.0 / np.cosh(0.5 * x), np.tanh(0.5 * x)
            V[:, 0, 0], V[:, 2, 2] = 0.02 * t, -0.02 * t
            V[:, 0, 1] = V[:, 1, 0] = V[:, 1, 2] = V[:, 2, 1] = 0.005 * g
            F[:, 0, 0], F[:, 2, 2] = -0.02 * 0.8 * (1.0 - t * t), 0.02 * 0.8 * (1.0 - t * t)
            F[:, 0, 1] = F[:, 1, 0] = F[:, 1, 2] = F[:, 2, 1] = 0.005 * 0.5 * g * th
        else:
            raise ValueError(model)
        return V, F
    return fun


def table(tab):
    """table_diabatic_n for a tests/pes_table_numpy.Table (or anything with x_first, dx, V, dV): the nodes are the table's doubles, the
    interpolation is x's dtype, in the header's operation order"""
    def fun(x):
        ty = x.dtype.type
        Vt, dVt = tab.V.astype(x.dtype), tab.dV.astype(x.dtype)
        mt = (tab.dx * tab.dV).astype(x.dtype)  # formed once in float64, as the library does when the model is defined
        n, x_first, dx = Vt.shape[0], ty(tab.x_first), ty(tab.dx)
        s = (x - x_first) / dx
        k = np.clip(np.floor(s), 0, n - 2).astype(np.int64)
        t = (s - k)[:, None, None]
        v0, v1, m0, m1 = Vt[k], Vt[k + 1], mt[k], mt[k + 1]
        delta = v1 - v0
        c2, c3 = 3.0 * delta - (2.0 * m0 + m1), (m0 + m1) - 2.0 * delta
        V = v0 + t * (m0 + t * (c2 + t * c3))
        dV = (m0 + t * (2.0 * c2 + 3.0 * t * c3)) / dx
        for mask, node in ((s < 0, 0), (s > n - 1, n - 1)):
            if mask.any():
                h = (x[mask] - (x_first + dx * node))[:, None, None]
                V[mask], dV[mask] = Vt[node] + dVt[node] * h, dVt[node]
        return V, -dV
    return fun


def jacobi(A):
    """jacobi_eig of csrc/gple_pes_n.h for A (m, N, N) symmetric: (lam (m, N) ascending, W (m, N, N), eigenvectors in the columns)"""
    A = np.array(A)
    m, N = A.shape[0], A.shape[1]
    one, zero = A.dtype.type(1), A.dtype.type(0)
    W = np.zeros_like(A)
    W[:, np.arange(N), np.arange(N)] = one
    for _ in range(8):
        for p in range(N - 1):
            for q in range(p + 1, N):
                apq = A[:, p, q].copy()
                on = apq != 0
                if not on.any():
                    continue
                with np.errstate(over="ignore"):
                    theta = (A[:, q, q] - A[:, p, p]) / (2.0 * np.where(on, apq, one))
                    t = np.where(theta >= 0, one, -one) / (np.abs(theta) + np.sqrt(theta * theta + one))
                c = one / np.sqrt(t * t + one)
                t, c, s = np.where(on, t, zero), np.where(on, c, one), np.where(on, t * c, zero)
                A[:, p, p] -= t * apq
                A[:, q, q] += t * apq
                A[:, p, q] = A[:, q, p] = zero
                for r in range(N):
                    if r != p and r != q:
                        arp, arq = A[:, r, p].copy(), A[:, r, q].copy()
                        A[:, r, p] = A[:, p, r] = c * arp - s * arq
                        A[:, r, q] = A[:, q, r] = s * arp + c * arq
                    wrp, wrq = W[:, r, p].copy(), W[:, r, q].copy()
                    W[:, r, p], W[:, r, q] = c * wrp - s * wrq, s * wrp + c * wrq
    lam = A[:, np.arange(N), np.arange(N)].copy()
    for i in range(N - 1):
        for j in range(i + 1, N):
            swap = lam[:, j] < lam[:, i]
            if swap.any():
                li, lj = lam[:, i].copy(), lam[:, j].copy()
                lam[:, i], lam[:, j] = np.where(swap, lj, li), np.where(swap, li, lj)
                wi, wj = W[:, :, i].copy(), W[:, :, j].copy()
                W[:, :, i], W[:, :, j] = np.where(swap[:, None], wj, wi), np.where(swap[:, None], wi, wj)
    return lam, W


def sign_convention(C):
    """adiabatic_sign_n: the last non-zero component of every column positive"""
    C = C.copy()
    N = C.shape[1]
    last = np.zeros((C.shape[0], N), dtype=C.dtype)
    for i in range(N):
        last = np.where(C[:, i, :] != 0, C[:, i, :], last)
    return np.where((last < 0)[:, None, :], -C, C)


def states(x, potential, flip=False):
    """V, E, C, F = C^T Fd C (symmetrised) at x (m,); flip: every eigenvector with the other sign"""
    V, Fd = potential(x)
    E, C = jacobi(V)
    C = sign_convention(C)
    if flip:
        C = -C
    A = np.swapaxes(C, 1, 2) @ (Fd @ C)
    return V, E, C, 0.5 * (A + np.swapaxes(A, 1, 2))


def complex_of(dtype):
    return np.result_type(dtype, np.complex64)


def uniforms(index, counter123, seed):
    """unit53 of the words (0, 1) and (2, 3) of Philox4x32-10, counter (index, *counter123), key (seed low, seed high); float64, exact"""
    index = np.asarray(index, dtype=np.uint64)
    ctr = np.stack([index & np.uint64(0xFFFFFFFF)] + [np.full_like(index, int(w) & 0xFFFFFFFF) for w in counter123], axis=-1)
    w = philox4x32(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)).astype(np.uint64)
    unit = lambda hi, lo: (((hi << np.uint64(32)) | lo) >> np.uint64(11)).astype(np.float64) * (1.0 / TWO53)
    return unit(w[..., 0], w[..., 1]), unit(w[..., 2], w[..., 3])


def sample(potential, num_pes, n, seed, x0, p0, sigma_x, sigma_p, surface0=0, trajectory_offset=0, dtype=np.float64):
    """gple_hop_sample -> (x, p, b, surface, status)"""
    ty = np.dtype(dtype).type
    u0, u1 = uniforms(trajectory_offset + np.arange(n), (0, 1, 0), seed)
    u0, u1 = u0.astype(dtype), u1.astype(dtype)
    rho = np.sqrt(-2.0 * np.log(1.0 - u0))
    angle = (8.0 * np.arctan(ty(1))) * u1  # cospi(2 u1), sinpi(2 u1)
    x, p = ty(x0) + ty(sigma_x) * rho * np.cos(angle), ty(p0) + ty(sigma_p) * rho * np.sin(angle)
    _, _, C, _ = states(x, potential)
    return x, p, C[:, :, surface0].astype(complex_of(dtype)), np.full(n, surface0, dtype=np.int32), np.zeros(n, dtype=np.int32)


def evolve(potential, state, seed, mass, dt, first_step, n_steps, x_left, x_right, reverse=False, trajectory_offset=0, flip=False):
    """gple_hop_evolve on a copy of the ensemble, in the dtype of its x -> (state, diagnostics): per trajectory hops, frustrated (counts),
    margin = the least |xi - (g_1 + ... + g_k)| over its steps and every k, ratio = the least |r| / p^2 where a hop was wanted, edge = the least
    |x_new - bound| for either bound (inf where there was none)"""
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
    Vx, _, _, Fx = states(x[live], potential, flip)
    for s in range(n_steps):
        step = first_step + s
        xs, ps, bs, a = x[live], p[live], b[live], surface[live].astype(np.int64)
        row = np.arange(len(live))
        # 1
        ps = ps + Fx[row, a, a] * dt / 2.0
        xn = xs + ps / mass * dt
        # 2
        Vn, E, C, F = states(xn, potential, flip)
        lam, W = jacobi(0.5 * (Vx + Vn))
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
        xi, _ = uniforms(trajectory_offset + live, (step & 0xFFFFFFFF, 0, step >> 32), seed)
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
        # 7
        diag["edge"][live] = np.minimum(diag["edge"][live], np.minimum(np.abs(xn - x_left), np.abs(xn - x_right)).astype(np.float64))
        out = np.where(xn < x_left, 1, np.where(xn > x_right, 2, 0))
        x[live], p[live], b[live], surface[live], status[live] = xn, ps, bs, a, out
        keep = out == 0
        live, Vx, Fx = live[keep], Vn[keep], F[keep]
        if len(live) == 0:
            break
    return (x, p, b, surface, status), diag


def observe_terms(potential, state, mass):
    """the (n, 4 N + 3) terms gple_hop_observe sums, in its order"""
    x, p, b, surface, status = state
    N, n = b.shape[1], len(x)
    _, E, C, _ = states(x, potential)
    c = np.einsum("mik,mi->mk", C, b)
    terms = np.zeros((n, 4 * N + 3), dtype=x.dtype)
    terms[np.arange(n), np.asarray(status) * N + np.asarray(surface)] = 1
    terms[:, 3 * N:4 * N] = c.real * c.real + c.imag * c.imag
    terms[:, 4 * N], terms[:, 4 * N + 1] = x, p
    terms[:, 4 * N + 2] = p * p / 2.0 / x.dtype.type(mass) + E[np.arange(n), np.asarray(surface)]
    return terms


def observe(potential, state, mass):
    return observe_terms(potential, state, mass).sum(axis=0)


class NumpyHopApi:
    """Api.hop_sample / hop_evolve / hop_observe on the restatement: potentials = {model id: function of builtin() or table()}; a built-in id
    that is not listed is made on demand"""

    def __init__(self, potentials=None, dtype=np.float64):
        self.potentials, self.dtype = dict(potentials or {}), dtype
        self.calls = []

    def _potential(self, num_pes, model):
        if model not in self.potentials:
            self.potentials[model] = builtin(model, num_pes)
        return self.potentials[model]

    def hop_sample(self, num_pes, model, n, seed, x0, p0, sigma_x, sigma_p, surface0=0, trajectory_offset=0, device_out=False):
        self.calls.append(("sample", n))
        return sample(self._potential(num_pes, model), num_pes, n, seed, x0, p0, sigma_x, sigma_p, surface0, trajectory_offset, self.dtype)

    def hop_evolve(self, num_pes, model, state, seed, mass, dt, first_step, n_steps, x_left, x_right, reverse=False, trajectory_offset=0):
        self.calls.append(("evolve", first_step, n_steps))
        return evolve(self._potential(num_pes, model), state, seed, mass, dt, first_step, n_steps, x_left, x_right, reverse, trajectory_offset)[0]

    def hop_observe(self, num_pes, model, state, mass):
        self.calls.append(("observe",))
        return observe(self._potential(num_pes, model), state, mass).astype(np.float64)


def tolerance(D, q):
    """the bound of the device against the float64 restatement for a quantity q: 64 D + 1e-13 max(1, max|q|), D the largest distance between
    the float64 and the long double restatement for that quantity (the rounding floor; a wrong decision is an error of order one)"""
    return 64.0 * float(D) + 1e-13 * max(1.0, float(np.max(np.abs(q))))


class FunctionTable:
    """what table() needs of a tabulated model: x_first, dx, V, dV (n, N, N), from pes.tabulate's return value"""

    def __init__(self, x_first, dx, V, dV):
        self.x_first, self.dx, self.V, self.dV = float(x_first), float(dx), np.asarray(V, dtype=np.float64), np.asarray(dV, dtype=np.float64)
        self.num_pes = self.V.shape[1]


def scalar_function(potential):
    """fun(x) -> (V, dV / dx) at a scalar x, the argument of pes.tabulate, from a potential of builtin()"""
    def fun(x):
        V, F = potential(np.array([x], dtype=np.float64))
        return V[0], -F[0]
    return fun
