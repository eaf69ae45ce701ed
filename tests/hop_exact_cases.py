"""References for the trajectory methods of csrc/gple_hop.hip (fewest switches, Ehrenfest, SQC, MASH) that owe nothing to their numpy
restatements ("Against closed forms and an ODE solution") — a helper, not collected by pytest.  Two parts.

The first part is numpy alone and knows no step of the library's: closed forms in numpy.longdouble on V = k x^2 / 2 I + A + B x, and a plain RK4
of the published equations  dx/dt = p / m,  dp/dt = f(x, b),  i db/dt = V(x) b  (hbar = 1) with one generic right-hand side.

  A1, B = 0, A full and symmetric.  Fd = -V' = -k x I, so every method's force is a multiple of -k x:
        fewest switches, MASH   C_a^T Fd C_a = -k x        (C_a a unit vector)
        Ehrenfest               b^dagger Fd b = -k x       (|b| = 1, kept by the unitary step)
        SQC                     b^dagger Fd b - gamma tr Fd = -k x (|b|^2 - gamma N): the harmonic force with the spring constant
                                k_eff = k (|b|^2 - gamma N) of the trajectory, |b|^2 being a constant of the motion (the step is unitary) and no
                                1 for the mapping amplitudes; the mid-point matrix keeps the k of the table.
      The kick-drift-kick step is the linear map K(dt / 2) D(dt) K(dt / 2) on (x, p), exact down to the step itself; the mid-point matrix is
      A + k (x^2 + x_new^2) / 4 I, which commutes with itself at every step, hence b_K = exp(-i phi) exp(-i A K dt) b_0 with
      phi = (k dt / 4) sum_s (x_s^2 + x_{s+1}^2).  exp(-i A K dt) is a Taylor series with scaling and squaring in long double: no eigen-solver.
  A2, A and B diagonal: uncoupled parabolas V_dd = k x^2 / 2 + A_dd + B_dd x.  The adiabatic surface a is the diabat argsort(diag V)[a], the
      same everywhere in the box because no two entries cross there (asserted); the trajectory is the harmonic flow about -B_dd / k, b stays
      on d and turns by the trapezoidal sum of V_dd along the path.
  B,  Tully's dual avoided crossing and the three-state model (the smooth ones), stated here from their definitions with the derivative
      checked by differences in the host test; the force of `rhs` is b^dagger Fd b - gamma tr Fd, or C_a^T Fd C_a with C from numpy.linalg.eigh.

The second part names the cases and runs them once (lru_cache) for tests/test_hop_exact_host.py and tests/test_gpu_hop_exact.py alike.  It takes
from the restatements the sampled start states (Philox) and the float64 and long double runs whose distance from these references calibrates
the device's tolerance; the references themselves never call them."""
import functools

import numpy as np

from tests import exact_cases as EC
from tests import hop_mash_numpy as HA
from tests import hop_mf_numpy as HM
from tests import hop_numpy as HN
from tests import hop_sqc_numpy as HQ

LD, CLD = np.longdouble, np.clongdouble


# ================================================================================================================================================
# part one: numpy only
# ================================================================================================================================================
def expm(M, squarings=12, terms=24):
    """exp(M) of a small complex matrix in long double: Taylor series of M / 2^squarings, squared back"""
    M = np.asarray(M, dtype=CLD) / LD(2) ** squarings
    term = out = np.eye(M.shape[0], dtype=CLD)
    for j in range(1, terms):
        term = term @ M / LD(j)
        out = out + term
    for _ in range(squarings):
        out = out @ out
    return out


def kdk_path(x, p, k, centre, mass, dt, steps):
    """positions x_0 ... x_steps (steps + 1, n) and the last momenta under the map K(dt / 2) D(dt) K(dt / 2), K(t): p -= k (x - centre) t,
    D(t): x += p / mass t, as one 2 x 2 matrix per trajectory (k may be an array) applied `steps` times; long double"""
    x, p = np.asarray(x, dtype=LD), np.asarray(p, dtype=LD)
    k, mass, dt = np.broadcast_to(np.asarray(k, dtype=LD), x.shape), LD(mass), LD(dt)
    kick = np.stack([np.stack([np.ones_like(k), np.zeros_like(k)], -1), np.stack([-k * dt / 2, np.ones_like(k)], -1)], -2)  # (n, 2, 2)
    drift = np.array([[1, dt / mass], [0, 1]], dtype=LD)
    M = kick @ drift @ kick
    z = np.stack([x - LD(centre), p], -1)[:, :, None]
    path = [z[:, 0, 0]]
    for _ in range(steps):
        z = M @ z
        path.append(z[:, 0, 0])
    return np.stack(path) + LD(centre), z[:, 1, 0]


def a1_closed(x, p, b, A, k, mass, dt, steps, k_eff=None):
    """(x, p, b) after `steps` steps on k x^2 / 2 I + A from the closed form; k_eff: the spring constant of every trajectory (default k)"""
    path, p_end = kdk_path(x, p, k if k_eff is None else k_eff, 0.0, mass, dt, steps)
    phi = LD(k) * LD(dt) / 4 * (path[:-1] ** 2 + path[1:] ** 2).sum(axis=0)
    U = expm(-1j * np.asarray(A, dtype=CLD) * (LD(dt) * steps))
    b_end = (np.cos(phi) - 1j * np.sin(phi))[:, None] * (np.asarray(b, dtype=CLD) @ U.T)
    return path[-1], p_end, b_end


def crossings(A, B):
    """the points where two diagonal entries of A + B x meet (inf for parallel lines)"""
    a, b = np.diag(np.asarray(A, dtype=np.float64)), np.diag(np.asarray(B, dtype=np.float64))
    out = []
    for i in range(len(a)):
        for j in range(i + 1, len(a)):
            out.append(np.inf if b[i] == b[j] else -(a[i] - a[j]) / (b[i] - b[j]))
    return np.array(out)


def a2_closed(x, p, b, A, B, k, mass, dt, steps, surface, box):
    """(x, p, b, d) after `steps` steps from the adiabatic surface `surface` of the uncoupled parabolas; d is its diabat"""
    assert np.count_nonzero(A - np.diag(np.diag(A))) == 0 and np.count_nonzero(B - np.diag(np.diag(B))) == 0
    assert (np.abs(crossings(A, B)) > box).all(), "two surfaces cross inside the box"
    d = int(np.argsort(np.diag(A))[surface])  # the order at x = 0 is the order in the whole box
    a_dd, b_dd, k = LD(A[d, d]), LD(B[d, d]), LD(k)
    path, p_end = kdk_path(x, p, k, -b_dd / k, mass, dt, steps)
    v = k * path * path / 2 + a_dd + b_dd * path
    theta = LD(dt) * ((v[:-1] + v[1:]) / 2).sum(axis=0)
    b_end = np.zeros(np.shape(b), dtype=CLD)
    b_end[:, d] = np.asarray(b, dtype=CLD)[:, d] * (np.cos(theta) - 1j * np.sin(theta))
    return path[-1], p_end, b_end, d


def dac(x):
    """Tully's dual avoided crossing (J. Chem. Phys. 93, 1061 (1990), model B): V, dV / dx in x's dtype"""
    V, dV = (np.zeros(x.shape + (2, 2), dtype=x.dtype) for _ in range(2))
    a, b, c, d, e0 = 0.10, 0.28, 0.015, 0.06, 0.05
    well, coupling = a * np.exp(-b * x * x), c * np.exp(-d * x * x)
    V[:, 1, 1], dV[:, 1, 1] = e0 - well, 2 * b * x * well
    V[:, 0, 1] = V[:, 1, 0] = coupling
    dV[:, 0, 1] = dV[:, 1, 0] = -2 * d * x * coupling
    return V, dV


def tsac(x):
    """the three-state model of csrc/gple_pes_n.h: V_00 = -V_22 = 0.02 tanh(0.8 x), V_11 = 0, V_01 = V_12 = 0.005 sech(0.5 x)"""
    V, dV = (np.zeros(x.shape + (3, 3), dtype=x.dtype) for _ in range(2))
    V[:, 0, 0] = 0.02 * np.tanh(0.8 * x)
    V[:, 2, 2] = -V[:, 0, 0]
    dV[:, 0, 0] = 0.02 * 0.8 / np.cosh(0.8 * x) ** 2
    dV[:, 2, 2] = -dV[:, 0, 0]
    coupling = 0.005 / np.cosh(0.5 * x)
    slope = -0.5 * coupling * np.tanh(0.5 * x)
    for i, j in ((0, 1), (1, 0), (1, 2), (2, 1)):
        V[:, i, j], dV[:, i, j] = coupling, slope
    return V, dV


MEAN, SURFACE = 0, 1


def rhs(potential, mass, kind, surface, gamma, x, p, b):
    """(dx/dt, dp/dt, db/dt).  kind MEAN: f = b^dagger Fd b - gamma tr Fd (Ehrenfest at gamma = 0, the Meyer-Miller force of include/gple.h
    otherwise); kind SURFACE: f = C_a^T Fd C_a on the adiabatic surface a = surface[i], C from numpy.linalg.eigh"""
    V, dV = potential(x)
    if kind == MEAN:
        f = gamma * np.einsum("mii->m", dV) - np.einsum("mi,mij,mj->m", np.conj(b), dV, b).real
    else:
        C = np.linalg.eigh(V.astype(np.float64))[1][np.arange(len(x)), :, surface].astype(x.dtype)
        f = -np.einsum("mi,mij,mj->m", C, dV, C)
    return p / mass, f, -1j * np.einsum("mij,mj->mi", V, b)


def rk4(potential, mass, kind, surface, gamma, x, p, b, t_end, h):
    """the classical fourth-order Runge-Kutta scheme over [0, t_end] at step h, in long double"""
    y = (np.asarray(x, dtype=LD), np.asarray(p, dtype=LD), np.asarray(b, dtype=CLD))
    n, h = int(round(t_end / h)), LD(h)
    assert n * h == t_end
    f = lambda y: rhs(potential, LD(mass), kind, surface, LD(gamma), *y)
    shift = lambda y, k, s: tuple(u + s * v for u, v in zip(y, k))
    for _ in range(n):
        k1 = f(y)
        k2 = f(shift(y, k1, h / 2))
        k3 = f(shift(y, k2, h / 2))
        k4 = f(shift(y, k3, h))
        y = tuple(u + h / 6 * (a + 2 * b_ + 2 * c + d) for u, a, b_, c, d in zip(y, k1, k2, k3, k4))
    return y


# ================================================================================================================================================
# part two: the cases, on the restatements and on the references
# ================================================================================================================================================
SEED = 20250117
assert np.finfo(LD).eps < 1e-18  # or neither the references nor D calibrate anything
GAMMA = HQ.GAMMA[HQ.TRIANGLE]    # SQC runs with the triangle windows at their customary gamma = 1 / 3


def widen(state):
    x, p, b, surface, status = state
    return x.astype(LD), p.astype(LD), b.astype(CLD), surface, status


def sample(method, potential, num_pes, n, packet, surface0, dtype=np.float64):
    """the start of a method on the restatement: x and p are the same for all four, b and what it means differ"""
    if method == "sqc":
        return HQ.sample(potential, num_pes, n, SEED, *packet, surface0, HQ.TRIANGLE, GAMMA, dtype=dtype)
    if method == "mash":
        return HA.sample(potential, num_pes, n, SEED, *packet, surface0, dtype=dtype)
    return HN.sample(potential, num_pes, n, SEED, *packet, surface0, dtype=dtype)


def restate(method, potential, state, mass, dt, steps, left, right):
    """(state, diagnostics) of the method's restatement, in the dtype of the state"""
    if method == "fssh":
        return HN.evolve(potential, state, SEED, mass, dt, 0, steps, left, right)
    if method == "mf":
        return HM.evolve(potential, state, mass, dt, steps, left, right)
    if method == "sqc":
        return HQ.evolve(potential, state, mass, dt, steps, left, right, GAMMA, drift=False)
    return HA.evolve(potential, state, mass, dt, steps, left, right)


def distance(got, want):
    """[max |x - x'|, max |p - p'|, max |b - b'|], evaluated in long double"""
    return [float(np.abs(np.asarray(got[q], dtype=want[q].dtype) - want[q]).max()) for q in range(3)]


# ---- part A ------------------------------------------------------------------------------------------------------------------------------------
A_K = A_MASS = 1.0
A_DT, A_STEPS, A_BOX, A_N = 0.05, 200, 6.0, 293
A_SIGMA = 2.0 ** -0.5
A_TABLE = (-8.0, 1.0 / 16.0, 257)
A1_X0, A2_X0 = 2.0, 1.0
A1_A = {2: np.array([[0.5, 0.3], [0.3, -0.5]]), 3: np.array([[0.5, 0.3, 0.1], [0.3, -0.2, 0.25], [0.1, 0.25, -0.9]])}
A2_A = {2: np.diag([5.0, -5.0]), 3: np.diag([6.0, 0.0, -6.0])}
A2_B = {2: np.diag([0.5, -0.5]), 3: np.diag([0.5, -0.25, -0.5])}
A1_METHODS = [("fssh", 2), ("fssh", 3), ("mf", 2), ("mf", 3), ("sqc", 2), ("sqc", 3), ("mash", 2)]
MASH_MARGIN = 1e-10
# what the float64 restatements may lie from the closed forms on the CPU (asserted in tests/test_hop_exact_host.py): the largest figure
# measured per group of cases over x, p and b, times HOST_MARGIN
HOST_MARGIN = 4.0
A_HOST = {"A1 fssh": 2.1e-13, "A1 mash": 2.1e-13, "A1 mf": 1.1e-12, "A1 sqc": 3.0e-12, "A2": 4.3e-14}


@functools.lru_cache(maxsize=None)
def a_table(which, num_pes):
    """the table of a part A family: what Api.pes_define takes, and the restatement's potential on it"""
    A = (A1_A if which == "A1" else A2_A)[num_pes]
    B = np.zeros_like(A) if which == "A1" else A2_B[num_pes]
    x_first, dx, n = A_TABLE
    V, dV = EC.quadratic_table(num_pes, A_K, A, B, x_first, dx, n)
    return (x_first, dx, V, dV), HN.table(HN.FunctionTable(x_first, dx, V, dV))


def a1_start(method, num_pes, state=None):
    """the ensemble of an A1 run.  Fewest switches and Ehrenfest: hop_sample's with b replaced by random normalised complex vectors, a true
    superposition; SQC and MASH keep the amplitudes of their own samples (state: the sample to use instead of the restatement's)"""
    _, potential = a_table("A1", num_pes)
    x, p, b, surface, status = sample(method, potential, num_pes, A_N, (A1_X0, 0.0, A_SIGMA, A_SIGMA), 0) if state is None else state
    if method in ("fssh", "mf"):
        rng = np.random.default_rng(20250117 + num_pes)
        b = rng.normal(size=b.shape) + 1j * rng.normal(size=b.shape)
        b = b / np.sqrt((np.abs(b) ** 2).sum(axis=1))[:, None]
    return x, p, b, surface, status


def a1_reference(method, num_pes, start):
    """the closed form from `start`, the float64 restatement's run from it with its diagnostics, and D per quantity"""
    _, potential = a_table("A1", num_pes)
    x, p, b = widen(start)[:3]
    k_eff = A_K * ((np.abs(b) ** 2).sum(axis=1) - LD(GAMMA) * num_pes) if method == "sqc" else None
    want = a1_closed(x, p, b, A1_A[num_pes], A_K, A_MASS, A_DT, A_STEPS, k_eff)
    end, diag = restate(method, potential, start, A_MASS, A_DT, A_STEPS, -A_BOX, A_BOX)
    return dict(want=want, end=end, diag=diag, D=distance(end, want))


@functools.lru_cache(maxsize=None)
def a1_case(method, num_pes):
    """an A1 run from the restatement's sample: (start, reference)"""
    start = a1_start(method, num_pes)
    return start, a1_reference(method, num_pes, start)


@functools.lru_cache(maxsize=None)
def a2_case(method, num_pes, surface0):
    """an A2 run: (start, reference as a1_reference's, with the diabat d)"""
    _, potential = a_table("A2", num_pes)
    start = sample(method, potential, num_pes, A_N, (A2_X0, 0.0, A_SIGMA, A_SIGMA), surface0)
    x, p, b = widen(start)[:3]
    *want, d = a2_closed(x, p, b, A2_A[num_pes], A2_B[num_pes], A_K, A_MASS, A_DT, A_STEPS, surface0, A_BOX)
    end, diag = restate(method, potential, start, A_MASS, A_DT, A_STEPS, -A_BOX, A_BOX)
    return start, dict(want=tuple(want), end=end, diag=diag, D=distance(end, want), d=d)


# ---- part B ------------------------------------------------------------------------------------------------------------------------------------
B_MASS, B_X0, B_BOX, B_N = 2000.0, -4.0, 50.0, 32
B_H, B_H_FINE = 1.0 / 8.0, 1.0 / 16.0
B_DTS = (1.0, 0.5)
B_MODELS = {"dac": (HN.DAC, 2, dac), "tsac": (HN.TSAC, 3, tsac)}
# name: model, p0, the time, the start surface
B_CASES = {"dac": dict(model="dac", p0=16.0, T=600.0, surface0=0),
           "tsac0": dict(model="tsac", p0=10.0, T=1000.0, surface0=0),
           "tsac2": dict(model="tsac", p0=14.0, T=800.0, surface0=2)}
# (case, method): every method where it exists (MASH has two levels); from the top surface Ehrenfest alone
B_RUNS = [("dac", "mf"), ("dac", "fssh"), ("dac", "sqc"), ("dac", "mash"), ("tsac0", "mf"), ("tsac0", "fssh"), ("tsac0", "sqc"), ("tsac2", "mf")]
B_RATIO = EC.RATIO          # second order: err(dt) / err(dt / 2), the window of §12
B_KEEP, B_MARGIN = 10, 1e-10  # the least number of trajectories that stay on their surface, and their least margin on the restatement
B_SELF = 1e-9               # the reference at h = 1 / 8 against h = 1 / 16, at most
B_SEES = 100.0              # err(dt = 1) over the bound of the Richardson combination, at least
# the self-convergence figures measured on the CPU (x, p, b), rounded up; the host test asserts them, the GPU test adds them to its bound
B_SELF_MEASURED = {("dac", "mf"): (3e-12, 1e-10, 1.3e-10), ("dac", "fssh"): (4e-15, 3e-14, 1.3e-10), ("dac", "sqc"): (6e-11, 3.5e-10, 2e-10),
                   ("dac", "mash"): (4e-15, 3e-14, 1.4e-10), ("tsac0", "mf"): (4e-13, 2.5e-12, 8e-12), ("tsac0", "fssh"): (3e-16, 2e-15, 8e-12),
                   ("tsac0", "sqc"): (2.5e-12, 2.5e-11, 9e-12), ("tsac2", "mf"): (2e-13, 8e-13, 4e-12)}


def b_start(case, method):
    c = B_CASES[case]
    model, num_pes, _ = B_MODELS[c["model"]]
    return sample(method, HN.builtin(model, num_pes), num_pes, B_N, (B_X0, c["p0"], 10.0 / c["p0"], c["p0"] / 20.0), c["surface0"])


@functools.lru_cache(maxsize=None)
def b_reference(case, method, h=B_H):
    """the RK4 solution (x, p, b) at the case's time from the method's float64 start, at step h"""
    c = B_CASES[case]
    x, p, b, surface, _ = b_start(case, method)
    kind = SURFACE if method in ("fssh", "mash") else MEAN
    return rk4(B_MODELS[c["model"]][2], B_MASS, kind, surface.astype(np.int64), GAMMA if method == "sqc" else 0.0, x, p, b, c["T"], h)


def richardson(coarse, fine):
    """(4 q(dt / 2) - q(dt)) / 3 per quantity: the second-order term of the splitting removed"""
    return tuple((4 * fine[q] - coarse[q]) / 3 for q in range(3))


@functools.lru_cache(maxsize=None)
def b_restated(case, method):
    """the case on the restatement at both time steps, float64 and long double: the runs, the trajectories that stay on their surface at both
    (all of them for Ehrenfest and SQC), and D per quantity: the distance of the float64 from the long double restatement, of the runs and of
    their Richardson combination (whose weights 4 / 3 and 1 / 3 it carries), the larger of the two"""
    c = B_CASES[case]
    model, num_pes, _ = B_MODELS[c["model"]]
    potential, start = HN.builtin(model, num_pes), b_start(case, method)
    keep, runs, wide = np.ones(B_N, dtype=bool), [], []
    for dt in B_DTS:
        steps = int(round(c["T"] / dt))
        end, diag = restate(method, potential, start, B_MASS, dt, steps, -B_BOX, B_BOX)
        far, _ = restate(method, potential, widen(start), B_MASS, dt, steps, -B_BOX, B_BOX)
        assert (end[4] == 0).all() and (far[4] == 0).all(), "somebody left"
        if method in ("fssh", "mash"):
            keep &= (diag["hops"] == 0) & (diag["frustrated"] == 0) & (diag["margin"] >= B_MARGIN) & (end[3] == start[3]) & (far[3] == start[3])
        runs.append(end)
        wide.append(far)
    cut = lambda s: tuple(a[keep] for a in s[:3])
    D = np.maximum(np.maximum(distance(cut(runs[0]), cut(wide[0])), distance(cut(runs[1]), cut(wide[1]))),
                   distance(richardson(cut(runs[0]), cut(runs[1])), richardson(cut(wide[0]), cut(wide[1]))))
    return dict(start=start, keep=keep, runs=runs, D=[float(d) for d in D])


def b_errors(case, method, runs, keep, reference=None):
    """(err(dt = 1), err(dt = 0.5), residual of the Richardson combination) per quantity of two runs against the reference, over `keep`"""
    ref = tuple(a[keep] for a in (b_reference(case, method) if reference is None else reference))
    cut = lambda s: tuple(np.asarray(a)[keep] for a in s[:3])
    coarse, fine = cut(runs[0]), cut(runs[1])
    return distance(coarse, ref), distance(fine, ref), distance(richardson(coarse, fine), ref)


def b_bound(case, method, self_convergence):
    """the bound of the device's Richardson combination per quantity, from the references only: twice the float64 restatement's own residual
    (the fourth-order remainder is deterministic and shared, the device adds rounding), plus tolerance(D_q, q), plus the reference's own error"""
    r = b_restated(case, method)
    residual = b_errors(case, method, r["runs"], r["keep"])[2]
    ref = b_reference(case, method)
    return [2.0 * residual[q] + HN.tolerance(r["D"][q], ref[q]) + self_convergence[q] for q in range(3)]


# ---- part C ------------------------------------------------------------------------------------------------------------------------------------
C_P0, C_DT, C_N, C_EVERY, C_LAST, C_SIGMA, C_SIGMAS = 30.0, 1.0, 2048, 50, 300, 1e-9, 5.0
