"""Independent numpy restatement of the energy-resolved spectrum of one absorbing run (gple_dvr_spectrum; DESIGN.md §11, "The spectrum of one
packet") for the tests — a helper, not collected by pytest.  It builds on tests/dvr_absorbing_numpy.py and tests/dvr_flux_numpy.py.  With
P = P4(A), psi_k = P^k psi0, theta = E dt / hbar and K = 2^J:
    product form    Y(E) = prod_{j < J} (I + e^{i theta 2^j} P^(2^j)) psi0 in complex128, a column per energy, the products as four real ones
                    (AN.cmul) in the library's order: R = P; per level Y += R (Y o e^{i theta 2^j}), R = R R
    density         a_c(E) = Re[(Pi_c Y)^H Y - (P Pi_c Y)^H (P Y)], the projection in the operation order of the library's mix
    oracle          long double, no matrix: psi is stepped with RK4 and sum_k e^{i theta k} psi_k accumulated with long-double cos and sin of theta k;
                    a_c = Re <Pi_c Y, Y> - Re <step(Pi_c Y), step(Y)>, the device of dvr_flux_numpy.oracle
    run_spectrum    the addition to the driver's loop: the levels, the default energies, the scaling of exact.run(spectrum=...)"""
import functools
import math

import numpy as np

from tests import dvr_absorbing_numpy as AN
from tests import dvr_flux_numpy as FN

EPS = AN.EPS
HBAR = AN.HBAR
LEVELS = (0, 1, 3, 6, 10)
LARGE_LEVELS = 5
N_E = {0: 17, 1: 5, 3: 16, 6: 70, 10: 64}  # the general energies of a shared shape at J levels; the large shape takes 5
CASES = [(shape, J) for shape in AN.SHAPES for J in LEVELS] + [(AN.LARGE, LARGE_LEVELS)]


def thetas(energies, dt):
    """theta = E dt / hbar as the library rounds it"""
    return np.asarray(energies, dtype=np.float64) * dt / HBAR


# ---- the product form in complex128 ---------------------------------------------------------------------------------------------------------------
def product_form(P, psi0, energies, dt, J):
    """(Y (dim, n_E), P^(2^J)): the phase of level j is cos and sin of theta 2^j (an exact product), never a squared z"""
    th = thetas(energies, dt)
    Y = np.repeat(np.asarray(psi0, dtype=np.complex128)[:, None], len(th), axis=1)
    R = P
    for j in range(J):
        if j:
            R = AN.cmul(R, R)
        t = th * 2.0 ** j
        Y = Y + AN.cmul(R, Y * (np.cos(t) + 1j * np.sin(t))[None, :])
    return Y, (AN.cmul(R, R) if J else P)


def project(basis, n_left, c, V):
    """Pi_c V for V (dim, m) in the library's order: row (m, a) = sum_j (b(a; m, k) b(a; j, k)) V((j, a))"""
    n, N = basis.shape[0], basis.shape[1]
    side, k = divmod(c, N)
    mask = ((np.arange(n) < n_left) == (side == 0)).astype(basis.dtype)
    b = basis[:, :, k] * mask[:, None]  # (n, N), zero off the side
    v = V.reshape(N, n, -1)
    out = np.zeros_like(v)
    for m in range(N):
        for j in range(N):
            out[m] = out[m] + (basis[:, m, k] * b[:, j])[:, None] * v[j]
    return out.reshape(V.shape)


def density(P, Y, basis, n_left):
    """a_c(E) (n_E, 2 num_pes): Re[Q^H Y - (P Q)^H (P Y)] with Q = Pi_c Y; no D_c is formed"""
    PY = AN.cmul(P, Y)
    out = np.empty((Y.shape[1], 2 * basis.shape[1]))
    for c in range(out.shape[1]):
        Q = project(basis, n_left, c, Y)
        PQ = AN.cmul(P, Q)
        out[:, c] = np.sum((Q.conj() * Y).real - (PQ.conj() * PY).real, axis=0)
    return out


def restated(H, W, num_pes, dt, psi0, energies, J, basis, n_left):
    """(Y, a, |P^K psi0|^2) of the restatement"""
    P = AN.p4(AN.generator(H, W, num_pes, dt))
    Y, RK = product_form(P, psi0, energies, dt, J)
    left = RK @ psi0
    return Y, density(P, Y, basis, n_left), float(np.vdot(left, left).real)


# ---- the oracle: long-double RK4 stepping, no matrix ------------------------------------------------------------------------------------------------
def _stepper(H, W, num_pes, dt):
    """step(u) for u (dim, 2 m) long double, the columns (re_0 .. re_m, im_0 .. im_m): one classical RK4 step of every column"""
    ld = np.longdouble
    Hl = np.asarray(H, dtype=ld)
    w = (np.zeros(H.shape[0], dtype=ld) if W is None else np.tile(W, num_pes).astype(ld))[:, None]
    h = ld(dt)

    def gen(u):  # -(W + i H)(a + i b) = (-W a + H b) + i (-W b - H a)
        m = u.shape[1] // 2
        Hu = Hl @ u
        return np.concatenate([-w * u[:, :m] + Hu[:, m:], -w * u[:, m:] - Hu[:, :m]], axis=1) / ld(HBAR)

    def step(u):
        k1 = gen(u)
        k2 = gen(u + h / 2 * k1)
        k3 = gen(u + h / 2 * k2)
        k4 = gen(u + h * k3)
        return u + h / 6 * (k1 + 2 * k2 + 2 * k3 + k4)

    return step


def trajectory(H, W, num_pes, dt, psi0, K):
    """psi_k for k <= K, long double: (re (K + 1, dim), im (K + 1, dim))"""
    step = _stepper(H, W, num_pes, dt)
    u = np.stack([psi0.real, psi0.imag], axis=1).astype(np.longdouble)
    re, im = [u[:, 0]], [u[:, 1]]
    for _ in range(K):
        u = step(u)
        re.append(u[:, 0]), im.append(u[:, 1])
    return np.array(re), np.array(im)


def oracle(H, W, num_pes, dt, traj, energies, J, basis, n_left):
    """from the trajectory: Y (dim, n_E) complex long double, a (n_E, 2 num_pes) long double, S = sum_{k < K} |psi_k|, |psi_K|^2"""
    ld = np.longdouble
    re, im = traj
    K, C = 2 ** J, 2 * num_pes
    th = thetas(energies, dt).astype(ld)
    k = np.arange(K, dtype=ld)
    angle = k[:, None] * th[None, :]  # theta k: exact in the 64-bit significand for k < 2^10
    cs, sn = np.cos(angle), np.sin(angle)
    Yr = re[:K].T @ cs - im[:K].T @ sn
    Yi = re[:K].T @ sn + im[:K].T @ cs
    S = float(np.sum(np.sqrt(np.sum(re[:K] ** 2 + im[:K] ** 2, axis=1))))
    bl = np.asarray(basis, dtype=ld)
    n_E = len(th)
    cols_r = [Yr] + [FN.project(bl, n_left, c, Yr) for c in range(C)]
    cols_i = [Yi] + [FN.project(bl, n_left, c, Yi) for c in range(C)]
    u = np.concatenate(cols_r + cols_i, axis=1)  # (dim, 2 (1 + C) n_E)
    half = (1 + C) * n_E
    inner = lambda v: np.array([np.sum(v[:, (1 + c) * n_E:(2 + c) * n_E] * v[:, :n_E] + v[:, half + (1 + c) * n_E:half + (2 + c) * n_E] * v[:, half:half + n_E], axis=0)
                                for c in range(C)]).T  # Re <u_c, u_0> per energy
    a = inner(u) - inner(_stepper(H, W, num_pes, dt)(u))
    return Yr + 1j * Yi, a, S, float(np.sum(re[K] ** 2 + im[K] ** 2))


# ---- the shared cases ---------------------------------------------------------------------------------------------------------------------------------
def general_energies(n_E):
    """total energies around the packet's p0^2 / 2m = 0.1; from five on, one negative and one far out (theta 2^j large: the range reduction of sincos)"""
    E = np.linspace(0.05, 0.15, n_E) if n_E > 1 else np.array([0.1])
    if n_E >= 5:
        E[1], E[-2] = -0.3, 37.7
    return E


def full_period_energies(K, dt):
    """theta_m = 2 pi m / K: dt is a power of two, so E = theta hbar / dt and back are exact"""
    return 2.0 * math.pi * np.arange(K) / K * HBAR / dt


@functools.lru_cache(maxsize=None)
def shape_trajectory(num_pes, n, with_absorber=True):
    c = FN.case(num_pes, n, with_absorber)
    K = 2 ** (LARGE_LEVELS if (num_pes, n) == AN.LARGE else max(LEVELS))
    traj = trajectory(c["H"], c["W"], num_pes, c["dt"], c["psi0"], K)
    for v in traj:
        v.setflags(write=False)
    return traj


@functools.lru_cache(maxsize=None)
def case(num_pes, n, J, which="general"):
    """one (shape, J, set of energies): the energies, the restatement and the oracle, and the tolerances the tests share.  which: "general"
    (N_E[J] energies), "period" (the 2^J full-period energies of the sum rule)"""
    c = FN.case(num_pes, n)
    if which == "period":
        E = full_period_energies(2 ** J, c["dt"])
    else:
        E = general_energies(5 if (num_pes, n) == AN.LARGE else N_E[J])
    return _evaluate(c, shape_trajectory(num_pes, n), E, J)


def _evaluate(c, traj, E, J, dt=None, W="case"):
    dt = c["dt"] if dt is None else dt
    W = c["W"] if isinstance(W, str) else W
    num_pes, dim = c["num_pes"], c["dim"]
    Y, a, left = restated(c["H"], W, num_pes, dt, c["psi0"], E, J, c["basis"], c["n_left"])
    Yo, ao, S, left_o = oracle(c["H"], W, num_pes, dt, traj, E, J, c["basis"], c["n_left"])
    e_ref = np.sqrt(np.sum(np.abs(Y.astype(np.clongdouble) - Yo) ** 2, axis=0)).astype(np.float64)  # per column
    e_ref_a = np.abs(a.astype(np.longdouble) - ao).astype(np.float64)                                # per (energy, channel)
    floor = EPS * math.sqrt(dim) * S
    out = dict(energies=E, J=J, K=2 ** J, S=S, Y=Y, a=a, remaining=left, Y_oracle=Yo, a_oracle=np.asarray(ao, dtype=np.float64), remaining_oracle=left_o,
               e_ref=e_ref, e_ref_a=e_ref_a, column_tolerance=8.0 * np.maximum(e_ref, floor), density_tolerance=8.0 * np.maximum(e_ref_a, floor * S))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def floor_density_tolerance(num_pes, n, J):
    """8 eps sqrt(dim) S^2, S from the trajectory alone: the density tolerance without the restatement's own distance (which can only widen it),
    for a case whose oracle densities would take too long (the 32 full-period energies of the large shape)"""
    re, im = shape_trajectory(num_pes, n)
    S = float(np.sum(np.sqrt(np.sum(re[:2 ** J] ** 2 + im[:2 ** J] ** 2, axis=1))))
    return 8.0 * EPS * math.sqrt(num_pes * n) * S * S


@functools.lru_cache(maxsize=None)
def flux_tolerance(num_pes, n, s):
    """FN.tolerance for any step count s: 8 max(e_ref, eps sqrt(dim) |psi0|^2) with e_ref the distance of the restated recurrence from the
    long-double stepping.  The large shape is stepped in long double to 37 only: its e_ref is left out, which asks more"""
    if s in (AN.LARGE_POWERS if (num_pes, n) == AN.LARGE else FN.POWERS):
        return FN.tolerance(num_pes, n, s)
    c = FN.case(num_pes, n)
    floor = EPS * math.sqrt(c["dim"]) * c["norm2"]
    if (num_pes, n) == AN.LARGE:
        return 8.0 * floor
    stepped = np.asarray(FN.oracle(c["H"], c["W"], num_pes, c["dt"], c["psi0"], (s,), c["basis"], c["n_left"])[s][0], dtype=np.float64)
    _, G = FN.matrices(num_pes, n, s)
    return 8.0 * max(float(np.abs(FN.forms(G, c["psi0"]) - stepped).max()), floor)


def state_tolerance(num_pes, n, J):
    """AN.tolerance for s = 2^J steps: 8 max(e_ref, eps sqrt(dim) |psi0|), e_ref the distance of the complex128 power applied to psi0 from psi_K
    of the long-double trajectory"""
    c = FN.case(num_pes, n)
    re, im = shape_trajectory(num_pes, n)
    K = 2 ** J
    U = AN.power(AN.p4(AN.generator(c["H"], c["W"], num_pes, c["dt"])), K)
    e = float(np.linalg.norm((U @ c["psi0"]).astype(np.clongdouble) - (re[K] + 1j * im[K])))
    return 8.0 * max(e, EPS * math.sqrt(c["dim"]) * float(np.linalg.norm(c["psi0"])))


@functools.lru_cache(maxsize=None)
def free_case(num_pes, n, J=3):
    """no absorber: dt so small that RK4's own loss over K steps is 1e-9 of the norm at most (the dt of the flux tests' W = NULL case), five energies"""
    c = FN.case(num_pes, n)
    normH = float(np.abs(np.linalg.eigvalsh(c["H"])).max())
    dt = (1e-9 * 120.0 / 2 ** J) ** 0.2 / normH
    traj = trajectory(c["H"], None, num_pes, dt, c["psi0"], 2 ** J)
    out = _evaluate(c, traj, general_energies(5), J, dt=dt, W=None)
    out.update(dt=dt, normH=normH)
    return out


# ---- the driver's addition ------------------------------------------------------------------------------------------------------------------------------
def levels_for(end_time, dt):
    """the smallest J with 2^J dt >= end_time"""
    J = 0
    while 2 ** J * dt < end_time:
        J += 1
    return J


def default_energies(s, lowest, n_E):
    """n_E momenta uniform in p0 +- 3 sigma_p (p0 alone for n_E = 1), E = p^2 / 2m + the lowest adiabatic energy at x0"""
    p = np.linspace(s["p0"] - 3.0 * s["sigma_p"], s["p0"] + 3.0 * s["sigma_p"], n_E) if n_E > 1 else np.array([s["p0"]])
    return p ** 2 / 2.0 / s["mass"] + lowest


def run_spectrum(s, num_pes, model, basis, adiabatic_energies, end_time, spectrum):
    """what exact.run(spectrum=...) adds after its loop, on this restatement: (rows (n_E, 1 + 2 num_pes) = E, rho_c(E); J; the population left after
    2^J steps)"""
    from tests import dvr_numpy as DN

    n, dx, x = s["n_grids"], s["dx"], s["x"]
    H = DN.hamiltonian(num_pes, model, DN.REFLECTIVE, x[0], dx, n, s["mass"])
    W = AN.absorber(x, s["mass"], s["xmin"], s["xmax"], s["absorbing_length"])
    n_left = int(np.sum(x < (s["xmin"] + s["xmax"]) / 2.0))
    g = DN.gaussian(x, s["x0"], s["p0"], s["sigma_x"])
    psi0 = np.concatenate([basis[:, j, 0] * g for j in range(num_pes)])
    J = levels_for(end_time, s["dt"])
    if isinstance(spectrum, (int, np.integer)):
        E = default_energies(s, float(np.min(adiabatic_energies[int(np.argmin(np.abs(x - s["x0"])))])), int(spectrum))
    else:
        E = np.asarray(spectrum, dtype=np.float64)
    _, a, left = restated(H, W, num_pes, s["dt"], psi0, E, J, basis, n_left)
    return np.concatenate([E[:, None], a * (dx * s["dt"] / (2.0 * math.pi * HBAR))], axis=1), J, left * dx
