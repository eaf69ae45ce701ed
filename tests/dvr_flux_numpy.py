"""Independent numpy restatement of what the absorber took (gple_dvr_flux, gple_dvr_flux_apply) for the tests — a helper, not
collected by pytest.  It builds on tests/dvr_absorbing_numpy.py: the channel projectors Pi_c (side of the box x adiabatic surface), the loss of
one step L = I - conj(P) P, the split D_c = (Pi_c L + L Pi_c) / 2, the recurrence G_c = sum_{k < s} conj(P^k) D_c P^k beside the binary power in
complex128 (products as four real ones, the library's order), and an oracle in long double that forms no matrix: per RK4 step the loss of
channel c is Re <Pi_c psi, psi> - Re <step(Pi_c psi), step(psi)>, which is psi^H D_c psi because conj(P) = P^H for the complex symmetric P."""
import functools
import math

import numpy as np

from tests import dvr_absorbing_numpy as AN

EPS = AN.EPS
HBAR = AN.HBAR
POWERS = (1,) + AN.POWERS  # 1, 2, 3, 37, 1000


# ---- channels: c = side num_pes + k; side 0 the grid points a < n_left, k the adiabatic state there (column k of basis (n, N, N)) --------------
def project(basis, n_left, c, v):
    """Pi_c v for v (dim,) or (dim, m), as the block-diagonal operation it is: per grid point on the side, b_k (b_k . v)"""
    n, N = basis.shape[0], basis.shape[1]
    side, k = divmod(c, N)
    mask = (np.arange(n) < n_left) == (side == 0)
    b = (basis[:, :, k] * mask[:, None]).astype(v.real.dtype)  # (n, N): b[a, j] = basis(a; j, k) on the side, 0 off it
    w = v.reshape((N, n) + v.shape[1:])
    tail = (None,) * (v.ndim - 1)
    coefficient = sum(b[:, j][(slice(None),) + tail] * w[j] for j in range(N))  # (n, ...)
    return np.stack([b[:, m][(slice(None),) + tail] * coefficient for m in range(N)]).reshape(v.shape)


def projectors(basis, n_left):
    """the dense Pi_c, real symmetric"""
    n, N = basis.shape[0], basis.shape[1]
    return [project(basis, n_left, c, np.eye(N * n)) for c in range(2 * N)]


def hermitian(Z):
    """the lower triangle and its mirror image: what the library keeps of a Hermitian product (the imaginary diagonal exactly zero)"""
    low = np.tril(Z, -1)
    return low + low.conj().T + np.diag(np.diag(Z).real)


def loss(P):
    """L = I - conj(P) P"""
    return hermitian(np.eye(P.shape[0]) - AN.cmul(P.conj(), P))


def channels(L, basis, n_left):
    """D_c = (Pi_c L + L Pi_c) / 2; L Pi_c = (Pi_c L)^H for the Hermitian L"""
    out = []
    for c in range(2 * basis.shape[1]):
        PL = project(basis, n_left, c, L.real) + 1j * project(basis, n_left, c, L.imag)
        out.append(hermitian(0.5 * (PL + PL.conj().T)))
    return out


def sandwich(R, X):
    """conj(R) (X R)"""
    return hermitian(AN.cmul(R.conj(), AN.cmul(X, R)))


def recurrence(P, D, s):
    """(P^s, [G_c]) left to right over the bits of s, beside the power: G += conj(R) (G R) before R = R R, G += conj(R) (D R) before R = R P"""
    R, G = P, list(D)
    for bit in bin(s)[3:]:
        G = [g + sandwich(R, g) for g in G]
        R = AN.cmul(R, R)
        if bit == "1":
            G = [g + sandwich(R, d) for g, d in zip(G, D)]
            R = AN.cmul(R, P)
    return R, G


def forms(G, psi):
    """Re psi^H G_c psi per channel"""
    return np.array([np.vdot(psi, g @ psi).real for g in G])


def flux_matrices(H, W, num_pes, dt, s, basis, n_left):
    """(U, [G_c]) of the restatement"""
    P = AN.p4(AN.generator(H, W, num_pes, dt))
    return recurrence(P, channels(loss(P), basis, n_left), s)


# ---- the oracle: long-double RK4 stepping of psi and of Pi_c psi, no matrix ----------------------------------------------------------------
def oracle(H, W, num_pes, dt, psi0, steps, basis, n_left):
    """{s: (absorbed per channel over s steps, psi after s steps)} for the ascending step counts `steps`, in long double"""
    ld = np.longdouble
    Hl, bl = np.asarray(H, dtype=ld), np.asarray(basis, dtype=ld)
    w = (np.zeros(H.shape[0], dtype=ld) if W is None else np.tile(W, num_pes).astype(ld))[:, None]
    h, C = ld(dt), 2 * num_pes

    def gen(u):  # -(W + i H) u / hbar on the columns (re_0 .. re_C, im_0 .. im_C)
        Hu = Hl @ u
        return np.concatenate([-w * u[:, :C + 1] + Hu[:, C + 1:], -w * u[:, C + 1:] - Hu[:, :C + 1]], axis=1) / ld(HBAR)

    def step(u):
        k1 = gen(u)
        k2 = gen(u + h / 2 * k1)
        k3 = gen(u + h / 2 * k2)
        k4 = gen(u + h * k3)
        return u + h / 6 * (k1 + 2 * k2 + 2 * k3 + k4)

    inner = lambda u: np.array([np.sum(u[:, 1 + c] * u[:, 0]) + np.sum(u[:, C + 2 + c] * u[:, C + 1]) for c in range(C)])  # Re <u_c, u_0>
    re, im = psi0.real.astype(ld), psi0.imag.astype(ld)
    total, out, done = np.zeros(C, dtype=ld), {}, 0
    for target in steps:
        for _ in range(target - done):
            u = np.stack([re] + [project(bl, n_left, c, re) for c in range(C)] + [im] + [project(bl, n_left, c, im) for c in range(C)], axis=1)
            before = inner(u)
            u = step(u)
            total = total + (before - inner(u))
            re, im = u[:, 0], u[:, C + 1]
        done = target
        out[target] = (total.copy(), re + 1j * im)
    return out


# ---- the shared cases: those of tests/dvr_absorbing_numpy.py with the adiabatic basis and the box's centre ------------------------------------
@functools.lru_cache(maxsize=None)
def case(num_pes, n, with_absorber=True):
    """AN.case plus basis, n_left (the grid points left of the box's centre), the oracle's figures `absorbed` {s: (2 num_pes,)} at the step
    counts the case has states for, and the restatement's matrices on demand (matrices(s))"""
    from oracle import evolve_oracle_n as ON

    c = dict(AN.case(num_pes, n, with_absorber))
    _, basis, _, _ = ON.adiabatic(c["x"], AN.MODEL[num_pes], num_pes)
    n_left = int(np.sum(c["x"] < (c["xmin"] + c["xmax"]) / 2.0))
    steps = AN.LARGE_POWERS if (num_pes, n) == AN.LARGE else POWERS
    got = oracle(c["H"], c["W"], num_pes, c["dt"], c["psi0"], steps, basis, n_left)
    c.update(basis=np.ascontiguousarray(basis), n_left=n_left, absorbed={s: np.asarray(v[0], dtype=np.float64) for s, v in got.items()},
             norm2=float(np.vdot(c["psi0"], c["psi0"]).real))
    return c


@functools.lru_cache(maxsize=None)
def matrices(num_pes, n, s, with_absorber=True):
    c = case(num_pes, n, with_absorber)
    U, G = flux_matrices(c["H"], c["W"], num_pes, c["dt"], s, c["basis"], c["n_left"])
    for m in [U] + G:
        m.setflags(write=False)
    return U, G


@functools.lru_cache(maxsize=None)
def e_ref(num_pes, n, s, with_absorber=True):
    """the largest channel difference between the complex128 recurrence applied to psi0 and the long-double oracle"""
    c = case(num_pes, n, with_absorber)
    _, G = matrices(num_pes, n, s, with_absorber)
    return float(np.abs(forms(G, c["psi0"]) - c["absorbed"][s]).max())


def tolerance(num_pes, n, s, with_absorber=True):
    """per channel: 8 max(e_ref, eps sqrt(dim) |psi0|^2): the restatement's own distance from the oracle, or the rounding of one quadratic form;
    the factor 8 allows for the MFMA's summation order (as AN.tolerance)"""
    c = case(num_pes, n, with_absorber)
    return 8.0 * max(e_ref(num_pes, n, s, with_absorber), EPS * math.sqrt(c["dim"]) * c["norm2"])


# ---- the SAC packet in the small box (AN.absorption_case): cumulative figures of the restatement after each application ------------------------
@functools.lru_cache(maxsize=None)
def absorption_case():
    a = dict(AN.absorption_case())
    n = a["n"]
    n_left = int(np.sum(a["x"] < (AN.SMALL["xmin"] + AN.SMALL["xmax"]) / 2.0))
    U, G = flux_matrices(a["H"], a["W"], 2, AN.DT, AN.ABSORPTION_STEPS, a["basis"], n_left)
    states = [a["psi0"]] + list(a["states"])
    cumulative = np.cumsum([forms(G, v) for v in states[:-1]], axis=0)  # after application k + 1: what the states 0 .. k lost
    stepped = oracle(a["H"], a["W"], 2, AN.DT, a["psi0"], (AN.ABSORPTION_STEPS,), a["basis"], n_left)[AN.ABSORPTION_STEPS][0]
    e = float(np.abs(forms(G, a["psi0"]) - np.asarray(stepped, dtype=np.float64)).max())
    a.update(n_left=n_left, G=G, cumulative=cumulative, e_ref_flux=e, basis=np.ascontiguousarray(a["basis"]))
    return a


def run_loop(s, num_pes, model, n_outputs, basis, until_absorbed=True):
    """the flux=True loop of exact.run on this restatement, from a set-up s of exact.setup(boundary=ABSORBING): records with `absorbed`
    (2, num_pes), and the stop (AN.run_loop's; with until_absorbed only "ABSORBED", at any <x>)"""
    from tests import dvr_numpy as DN

    n, dx, x = s["n_grids"], s["dx"], s["x"]
    H = DN.hamiltonian(num_pes, model, DN.REFLECTIVE, x[0], dx, n, s["mass"])
    W = AN.absorber(x, s["mass"], s["xmin"], s["xmax"], s["absorbing_length"])
    n_left = int(np.sum(x < (s["xmin"] + s["xmax"]) / 2.0))
    U, G = flux_matrices(H, W, num_pes, s["dt"], s["output_step"], basis, n_left)
    g = DN.gaussian(x, s["x0"], s["p0"], s["sigma_x"])
    psi = np.concatenate([basis[:, j, 0] * g for j in range(num_pes)])
    out, stop, absorbed = [], None, np.zeros((2, num_pes))
    last_x, old = s["x0"], np.zeros(num_pes)
    for k in range(n_outputs):
        ad = np.einsum("ajk,ja->ka", basis, psi.reshape(num_pes, n)).reshape(-1)
        pops = np.array([np.sum(np.abs(ad[m * n:(m + 1) * n]) ** 2) * dx for m in range(num_pes)])
        X = sum(np.dot(x, np.abs(psi[m * n:(m + 1) * n]) ** 2) for m in range(num_pes)) * dx
        out.append(dict(t=k * s["output_step"] * s["dt"], populations=pops, absorbed=absorbed.copy(), x=X))
        if until_absorbed:
            if pops.sum() < AN.PPL_LIM:
                stop = "ABSORBED"
                break
        elif X > 0.0:
            stop = ("OUT" if X > -s["x0"] else "REVERSED" if (X - last_x) * s["p0"] < 0 else "ABSORBED" if pops.sum() < AN.PPL_LIM
                    else "STABLE" if np.all(np.abs(pops - old) < 1e-5) else None)
            if stop:
                break
        last_x, old = X, pops
        absorbed = absorbed + forms(G, psi).reshape(2, num_pes) * dx
        psi = U @ psi
    return out, stop
