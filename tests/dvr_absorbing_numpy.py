"""Independent numpy restatement of the exact DVR dynamics with the absorbing boundary (general.h:88-93 of the reference's
schrodinger_equation/) for the tests — a helper, not collected by pytest.  Written from the formulas: the absorber of pes.cpp:64-93, the
classical RK4 step that general.cpp:233-236 documents on i hbar dpsi/dt = (H - i W) psi, its one-step propagator P4(A) with
A = -(W + i H) dt / hbar, and the binary power.  H comes from tests/dvr_numpy.hamiltonian (the reflective one, as the reference's switch
falls through to it)."""
import functools
import math

import numpy as np
from scipy.special import ellipk

from tests import dvr_numpy as DN

HBAR = 1.0
EPS = np.finfo(np.float64).eps
C_ABS = math.sqrt(2.0) * float(ellipk(0.5))  # sqrt(2) K(1 / sqrt(2)); scipy's parameter is m = k^2
PPL_LIM = 1e-4  # general.h:45


def absorber_terms(x, mass, xmin, xmax, length, literal=False):
    """(inside, pref, 1/(c - xi)^2, 1/(c + xi)^2, 2/c^2).  literal: the reference's own branch `x < xmin` (pes.cpp:91), which sends the grid
    point x == xmin down the right-hand side."""
    x = np.asarray(x, dtype=np.float64)
    left = (x < xmin) if literal else (x <= xmin)
    xi = C_ABS * np.where(left, x - xmin, x - xmax) / length
    pref = (2.0 * math.pi * HBAR / length) ** 2 * 2.0 / mass
    return (x > xmin) & (x < xmax), pref, 1.0 / (C_ABS - xi) ** 2, 1.0 / (C_ABS + xi) ** 2, 2.0 / C_ABS ** 2


def absorber(x, mass, xmin, xmax, length, literal=False):
    """W(x): 0 inside (xmin, xmax), pref (1/(c - xi)^2 + 1/(c + xi)^2 - 2/c^2) outside"""
    inside, pref, a, b, c = absorber_terms(x, mass, xmin, xmax, length, literal)
    return np.where(inside, 0.0, pref * (a + b - c))


def generator(H, W, num_pes, dt):
    """A = -(W + i H) dt / hbar; W (one value per grid point, or None) on every surface"""
    A = -1j * np.asarray(H, dtype=np.float64) * dt / HBAR
    if W is not None:
        A = A + np.diag(-np.tile(W, num_pes) * dt / HBAR)
    return A


def p4(A):
    """P4(A) = I + A (I + A/2 (I + A/3 (I + A/4))): exactly what one classical RK4 step applies for a constant generator"""
    I = np.eye(A.shape[0], dtype=A.dtype)
    Q = I + A / 4
    for k in (3, 2, 1):
        Q = I + (A / k) @ Q
    return Q


def cmul(X, Y):
    """the complex product as four real products, the order the library forms it in"""
    Xr, Xi, Yr, Yi = (np.ascontiguousarray(v) for v in (X.real, X.imag, Y.real, Y.imag))  # contiguous planes: the strided views miss BLAS
    return (Xr @ Yr - Xi @ Yi) + 1j * (Xr @ Yi + Xi @ Yr)


def power(P, s):
    """P^s, left to right over the bits of s: R = R R, then R = R P where the bit is set (complex128)"""
    R = P
    for bit in bin(s)[3:]:
        R = cmul(R, R)
        if bit == "1":
            R = cmul(R, P)
    return R


def rk4_states(H, W, num_pes, dt, psi0, steps):
    """psi after each of the step counts `steps` (ascending) of classical RK4 in long double:
    k1 = L psi, k2 = L (psi + dt/2 k1), k3 = L (psi + dt/2 k2), k4 = L (psi + dt k3), psi += dt/6 (k1 + 2 k2 + 2 k3 + k4), L = -(W + i H) / hbar.
    H psi is formed as one real long-double product with the two columns (Re psi, Im psi)."""
    ld = np.longdouble
    Hl = np.asarray(H, dtype=ld)
    w = np.zeros(H.shape[0], dtype=ld) if W is None else np.tile(W, num_pes).astype(ld)
    v = np.stack([psi0.real, psi0.imag], axis=1).astype(ld)  # (dim, 2)
    h = ld(dt)

    def L(u):
        Hu = Hl @ u
        return np.stack([-w * u[:, 0] + Hu[:, 1], -w * u[:, 1] - Hu[:, 0]], axis=1) / ld(HBAR)  # -(W + iH)(a + ib) = (-W a + H b) + i (-W b - H a)

    out, done = {}, 0
    for target in steps:
        for _ in range(target - done):
            k1 = L(v)
            k2 = L(v + h / 2 * k1)
            k3 = L(v + h / 2 * k2)
            k4 = L(v + h * k3)
            v = v + h / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
        done = target
        out[target] = v[:, 0] + 1j * v[:, 1]
    return out


def halve(dt, W):
    """the halving rule of exact.setup: dt is halved until dt max W / hbar <= 2 -> (dt, halvings)"""
    k = 0
    while W is not None and dt * float(np.max(W)) / HBAR > 2.0:
        dt, k = dt / 2.0, k + 1
    return dt, k


# ---- the small cases the tests share: n grid points at dx = 1/16 around 0, of which five on either side absorb ------------------------------
MASS, P0, SIGMA_P, DX, DT = 2000.0, 20.0, 1.0, 1.0 / 16.0, 1.0 / 8.0
LENGTH = 2.0 * math.pi * HBAR / (P0 - 3.0 * SIGMA_P)
N_ABS = int(LENGTH / DX)  # 5
SHAPES = [(2, 23), (2, 37), (3, 43), (2, 96)]  # dim 46 < 64, 74, 129 = 2 * 64 + 1, 192 = 3 * 64
MODEL = {2: 1, 3: 3}  # DAC at two levels, TSAC at three
POWERS = (2, 3, 37, 1000)
LARGE, LARGE_POWERS = (2, 531), (37,)  # dim 1062, ld 1088: the 64 x 64 GEMM of the library instead of its split-k one; stepped in long double to 37 only


@functools.lru_cache(maxsize=None)
def case(num_pes, n, with_absorber=True):
    """one shape: grid, box, H, W, dt after the halving rule, a wavepacket psi0 and the long-double RK4 states after POWERS steps"""
    x_first = -DX * (n - 1) / 2.0
    x = DN.grid(x_first, DX, n)
    xmin, xmax = float(x[N_ABS]), float(x[n - 1 - N_ABS])
    H = DN.hamiltonian(num_pes, MODEL[num_pes], DN.REFLECTIVE, x_first, DX, n, MASS)
    W = absorber(x, MASS, xmin, xmax, LENGTH) if with_absorber else None
    dt, halvings = halve(DT, W)
    g = DN.gaussian(x, -0.25, P0, HBAR / 2.0 / SIGMA_P / 4.0)
    psi0 = np.concatenate([g * (0.8 if m == 0 else 0.6 / math.sqrt(num_pes - 1) * 1j ** m) for m in range(num_pes)])
    states = rk4_states(H, W, num_pes, dt, psi0, LARGE_POWERS if (num_pes, n) == LARGE else POWERS)
    for v in states.values():
        v.setflags(write=False)
    return dict(num_pes=num_pes, n=n, dim=num_pes * n, x_first=x_first, x=x, xmin=xmin, xmax=xmax, H=H, W=W, dt=dt, halvings=halvings, psi0=psi0,
                states=states)


@functools.lru_cache(maxsize=None)
def reference_error(num_pes, n, s, with_absorber=True):
    """e_ref: the distance of the numpy complex128 power, applied to psi0, from the long-double stepping"""
    c = case(num_pes, n, with_absorber)
    U = power(p4(generator(c["H"], c["W"], num_pes, c["dt"])), s)
    return float(np.linalg.norm((U @ c["psi0"]).astype(np.clongdouble) - c["states"][s]))


def tolerance(num_pes, n, s, with_absorber=True):
    """8 max(e_ref, eps sqrt(dim) |psi0|): e_ref is the restatement's own distance from the stepping, the second term the rounding of one
    matrix-vector product; the factor 8 allows for the MFMA's summation order"""
    c = case(num_pes, n, with_absorber)
    return 8.0 * max(reference_error(num_pes, n, s, with_absorber), EPS * math.sqrt(c["dim"]) * float(np.linalg.norm(c["psi0"])))


# ---- the small scattering run: box [-3, 3] at dx = 1/16 (107 points, dim 214), the packet of exact.setup(**SMALL) ----------------------------
SMALL = dict(xmin=-3.0, xmax=3.0, dx=DX, mass=MASS, p0=P0, sigma_p=SIGMA_P, x0=-1.5, dt_max=DT)


def run_loop(s, num_pes, model, n_outputs, basis):
    """main.cpp:210-298 for the absorbing boundary on this restatement, from a set-up s of exact.setup(boundary=ABSORBING): per output a record
    (t, populations, E, x, psi) up to the stop, and which stop fired ("OUT", "REVERSED", "ABSORBED", "STABLE" or None), the criteria in the
    reference's order.  basis (n, N, N): the adiabatic states per grid point."""
    n, dx, x = s["n_grids"], s["dx"], s["x"]
    H = DN.hamiltonian(num_pes, model, DN.REFLECTIVE, x[0], dx, n, s["mass"])
    W = absorber(x, s["mass"], s["xmin"], s["xmax"], s["absorbing_length"])
    U = power(p4(generator(H, W, num_pes, s["dt"])), s["output_step"])
    g = DN.gaussian(x, s["x0"], s["p0"], s["sigma_x"])
    psi = np.concatenate([basis[:, j, 0] * g for j in range(num_pes)])
    out, last_x, old, stop = [], s["x0"], np.zeros(num_pes), None
    for k in range(n_outputs):
        ad = np.einsum("ajk,ja->ka", basis, psi.reshape(num_pes, n)).reshape(-1)
        pops = np.array([np.sum(np.abs(ad[m * n:(m + 1) * n]) ** 2) * dx for m in range(num_pes)])
        X = sum(np.dot(x, np.abs(psi[m * n:(m + 1) * n]) ** 2) for m in range(num_pes)) * dx
        out.append(dict(t=k * s["output_step"] * s["dt"], populations=pops, E=np.vdot(psi, H @ psi).real * dx, x=X, psi=psi, psi_adia=ad))
        if X > 0.0:
            stop = ("OUT" if X > -s["x0"] else "REVERSED" if (X - last_x) * s["p0"] < 0 else "ABSORBED" if pops.sum() < PPL_LIM
                    else "STABLE" if np.all(np.abs(pops - old) < 1e-5) else None)
            if stop:
                break
        last_x, old = X, pops
        psi = U @ psi
    return out, stop


ABSORPTION_STEPS, ABSORPTION_APPLICATIONS = 1600, 12  # 200 time units per application: the slow reflected part has left by the ninth


@functools.lru_cache(maxsize=None)
def absorption_case():
    """Tully's single avoided crossing in the small box: H, W, psi0 (the packet on the lower adiabatic surface), the restatement's propagator of
    ABSORPTION_STEPS steps, its states after 1 .. ABSORPTION_APPLICATIONS applications, and e_ref of one application"""
    from oracle import evolve_oracle_n as ON

    n = int((SMALL["xmax"] - SMALL["xmin"]) / DX) + 1 + 2 * N_ABS
    x = SMALL["xmin"] + DX * (np.arange(n) - N_ABS)
    H = DN.hamiltonian(2, 0, DN.REFLECTIVE, x[0], DX, n, MASS)
    W = absorber(x, MASS, SMALL["xmin"], SMALL["xmax"], LENGTH)
    _, basis, _, _ = ON.adiabatic(x, 0, 2)
    g = DN.gaussian(x, SMALL["x0"], P0, HBAR / 2.0 / SIGMA_P)
    psi0 = np.concatenate([basis[:, j, 0] * g for j in range(2)])
    U = power(p4(generator(H, W, 2, DT)), ABSORPTION_STEPS)
    states = [psi0]
    for _ in range(ABSORPTION_APPLICATIONS):
        states.append(U @ states[-1])
    stepped = rk4_states(H, W, 2, DT, psi0, (ABSORPTION_STEPS,))[ABSORPTION_STEPS]
    e_ref = float(np.linalg.norm(states[1].astype(np.clongdouble) - stepped))
    return dict(n=n, x=x, H=H, W=W, basis=basis, psi0=psi0, U=U, states=np.array(states[1:]), e_ref=e_ref)
