"""The family on which the MQCLE has no method error, V(x) = k x^2 / 2 I + A + B x with constant symmetric A and B, for the tests that set the
MQCLE propagator against the DVR solution and against a closed form — a helper of numpy and closed forms only, not collected by
pytest.  The Moyal expansion of the partial Wigner transform of -i [V, rho] stops after its first-order term on this family (the second-order
term is a commutator with V'' = k I, every higher derivative of V is zero), so the partial Wigner transform of the Schrödinger solution and the
MQCLE density are the same function of (x, p, t); with B = 0 and diagonal A every element follows the harmonic flow and turns at its own gap,
which is a closed form down to the Strang splitting itself.  hbar = 1 throughout."""
import math

import numpy as np

REFLECTIVE, PERIODIC = 0, 1
SX = np.array([[0.0, 1.0], [1.0, 0.0]])


def box(n, length):
    """n points over [-length / 2, length / 2): (grid, spacing); the period of the grid is n spacings"""
    d = length / n
    return -length / 2.0 + d * np.arange(n), d


def quadratic_table(num_pes, k, A, B, x_first, dx, n):
    """V, dV (n, num_pes, num_pes) of k x^2 / 2 I + A + B x at x_first + dx j: the arguments of Api.pes_define and tests/pes_table_numpy.Table"""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    assert A.shape == B.shape == (num_pes, num_pes) and np.array_equal(A, A.T) and np.array_equal(B, B.T)
    x = (x_first + dx * np.arange(n))[:, None, None]
    eye = np.eye(num_pes)[None]
    return 0.5 * k * x * x * eye + A[None] + B[None] * x, k * x * eye + B[None] + 0.0 * x


def strang_map(dt, mass, k, f):
    """the 2 x 2 forward map of one step on (x, p): drift(dt / 2) kick(dt) drift(dt / 2), the drift x += f p / mass t and the kick p -= f k x t.
    f = 1 for transform lengths of n spacings; the driver's lengths of n - 1 spacings scale every shift by f = n / (n - 1) (quirk 1 of §12)"""
    drift = np.array([[1.0, f * dt / 2.0 / mass], [0.0, 1.0]])
    kick = np.array([[1.0, 0.0], [-f * k * dt, 1.0]])
    return drift @ kick @ drift


def wigner_gauss(x, p, x0, p0, sigma):
    """the Wigner function of a Gaussian packet of position width sigma on the grid (x major, p fastest)"""
    return np.exp(-(x[:, None] - x0) ** 2 / (2.0 * sigma ** 2) - 2.0 * sigma ** 2 * (p[None, :] - p0) ** 2) / math.pi


def gaps_of(A):
    """gaps[a, b] = A_aa - A_bb of a diagonal A"""
    d = np.diag(np.asarray(A, dtype=np.float64))
    return d[:, None] - d[None, :]


def closed_form(x, p, x0, p0, sigma, M, K, gaps, t, weights=None):
    """rho_ab(x, p) = w_ab W_Gauss(M^-K (x, p)) exp(-i (A_aa - A_bb) t) after K steps of map M from rho_ab = w_ab W_Gauss: every element rides
    the same flow (the force -k x is the same on every surface) and Q commutes with it (the gaps do not depend on x).  weights: Hermitian
    (N, N), 1/2 everywhere when None.  -> (N, N, n_x, n_p) complex"""
    gaps = np.asarray(gaps, dtype=np.float64)
    w = np.full(gaps.shape, 0.5, dtype=complex) if weights is None else np.asarray(weights, dtype=complex)
    back = np.linalg.matrix_power(np.linalg.inv(np.asarray(M, dtype=np.float64)), K)
    xb = back[0, 0] * x[:, None] + back[0, 1] * p[None, :]
    pb = back[1, 0] * x[:, None] + back[1, 1] * p[None, :]
    g = np.exp(-(xb - x0) ** 2 / (2.0 * sigma ** 2) - 2.0 * sigma ** 2 * (pb - p0) ** 2) / math.pi
    return (w * np.exp(-1j * gaps * t))[:, :, None, None] * g[None, None]


def gaussian_state(x, x0, p0, sigma):
    """the packet of tests/dvr_numpy.gaussian, normalised on the grid"""
    psi = np.exp(-((x - x0) / 2.0 / sigma) ** 2 + 1j * p0 * x)
    return psi / math.sqrt(np.vdot(psi, psi).real * (x[1] - x[0]))


def rel(a, b):
    """max |a - b| over max |b|, over all elements"""
    return np.abs(a - b).max() / np.abs(b).max()


def richardson(coarse, fine):
    """(4 rho(dt / 2) - rho(dt)) / 3: the second-order term of the Strang splitting removed"""
    return (4.0 * fine - coarse) / 3.0


# ---- the closed form: B = 0, diagonal A with distinct gaps, every element a <= b populated ---------------------------------------------------
K_FORCE, MASS = 1.0, 1.0
CLOSED_DT, CLOSED_STEPS = 0.05, 50
CLOSED_X0, CLOSED_P0 = 2.0, 0.5
CLOSED_A = {2: np.diag([0.5, -0.5]), 3: np.diag([1.0, 0.3, -1.5])}  # gaps 1.0, and 0.7 / 1.8
CLOSED_W = {2: np.array([[0.6, 0.3 + 0.2j], [0.3 - 0.2j, 0.4]]),
            3: np.array([[0.5, 0.2 + 0.1j, -0.1 + 0.3j], [0.2 - 0.1j, 0.3, 0.25j], [-0.1 - 0.3j, -0.25j, 0.2]])}
# n: (box length, packet width).  The packet turns about the origin at radius 2.06 and its widths swing between sigma and 1 / (2 sigma); the
# box and the top bin pi / dx must both lie where it is below 1e-13 of its peak.  At n = 64 (dx = 0.25, top bin 12.6) sigma = 0.6 leaves
# exp(-(0.6 pi / 0.25)^2 / 2) = 4.5e-13 at the top bin, so that grid takes the round packet sigma = 1 / sqrt 2 (2e-17 there, 2e-14 at the edge)
CLOSED_GRIDS = {64: (16.0, math.sqrt(0.5)), 127: (16.0, 0.6), 128: (16.0, 0.6), 257: (20.0, 0.6), 300: (20.0, 0.6)}
# the project's own figure for gple_mqcl_evolve against its restatement (§12), relative to max |rho| over the whole state
CLOSED_TOL = 2e-12
# what the restatement alone may use of it on the CPU (asserted in tests/test_solvers_agree_host.py)
CLOSED_HOST = 0.1 * CLOSED_TOL


def closed_tables(num_pes, n):
    """{name: (x_first, dx, V, dV)}: one table whose nodes are the grid, one coarser (dx = 0.5) whose nodes lie off it; a cubic Hermite
    segment reproduces a quadratic exactly, so both are the same potential"""
    A, B = CLOSED_A[num_pes], np.zeros((num_pes, num_pes))
    x, dx = box(n, CLOSED_GRIDS[n][0])
    first = math.floor(x[0]) - 1.0 + 0.171875  # off the grid, below it
    m = int(math.ceil((x[-1] + 1.0 - first) / 0.5)) + 1
    return {"grid": (x[0], dx, *quadratic_table(num_pes, K_FORCE, A, B, x[0], dx, len(x))),
            "coarse": (first, 0.5, *quadratic_table(num_pes, K_FORCE, A, B, first, 0.5, m))}


def closed_case(num_pes, n, driver_lengths):
    """(x, p, lengths, f, start, expected) of one closed-form run: lengths of n spacings, or the driver's n - 1 (f = n / (n - 1))"""
    length, sigma = CLOSED_GRIDS[n]
    x, dx = box(n, length)
    p, dp = box(n, length)
    f = n / (n - 1.0) if driver_lengths else 1.0
    lengths = ((n - 1) * dx, (n - 1) * dp) if driver_lengths else (n * dx, n * dp)
    gaps = gaps_of(CLOSED_A[num_pes])
    args = (x, p, CLOSED_X0, CLOSED_P0, sigma, strang_map(CLOSED_DT, MASS, K_FORCE, f))
    start = closed_form(*args, 0, gaps, 0.0, CLOSED_W[num_pes])
    expected = closed_form(*args, CLOSED_STEPS, gaps, CLOSED_STEPS * CLOSED_DT, CLOSED_W[num_pes])
    return x, p, lengths, f, start, expected


# ---- DVR against MQCLE: coupled cases, a coherent packet on diabat 0 ---------------------------------------------------------------------------
PACKET_X0, PACKET_SIGMA, T_END = 2.0, math.sqrt(0.5), 2.0
DT_COARSE, DT_FINE = 0.02, 0.01
B3 = np.array([[0.2, 0.5, 0.0], [0.5, 0.0, 0.4], [0.0, 0.4, -0.2]])
# name: num_pes, n, box length (p_length: the p box where it is not the x box), A, B, and the figures of the restatements (tests/mqcl_numpy.py
# against tests/dvr_numpy.py) on the CPU, rounded up: `plain` bounds max |rho_MQCLE(dt = 0.01) - W[psi_DVR]| / max |W| over all elements,
# `richardson` the same for the combination of dt = 0.02 and 0.01, per boundary of the DVR Hamiltonian (reflective, periodic).  Measured:
#   two-96     3.9228e-5, 8.20e-9 / 8.20e-9      two-128    3.8981e-5, 8.28e-9 / 8.28e-9
#   three-128  3.5028e-5, 7.03e-9 / 1.02e-8      two-300    3.9210e-5, 8.20e-9 / 8.20e-9
# tests/test_solvers_agree_host.py asserts the two-level figures at n = 96 and 128 on every run; one step of the restatement costs 80 ms at
# three levels and 140 ms at n = 300 (300 steps a case), so those two rows were measured once with the same code and are recorded here
# (the conditions of all four cases are asserted there).  periodic_wigner: the box is wide enough for the periodic Wigner sum (below)
COUPLED = {
    "two-128": dict(num_pes=2, n=128, length=16.0, A=np.diag([0.5, -0.5]), B=0.5 * SX, plain=3.95e-5, richardson=(1.0e-8, 1.0e-8)),
    "two-96": dict(num_pes=2, n=96, length=16.0, A=np.diag([0.5, -0.5]), B=0.5 * SX, plain=3.97e-5, richardson=(1.0e-8, 1.0e-8)),
    "three-128": dict(num_pes=3, n=128, length=16.0, A=np.diag([0.8, 0.0, -0.6]), B=B3, plain=3.55e-5, richardson=(8.5e-9, 1.25e-8)),
    "two-300": dict(num_pes=2, n=300, length=30.0, p_length=24.0, A=np.diag([0.5, -0.5]), B=0.5 * SX, plain=3.97e-5, richardson=(1.0e-8, 1.0e-8),
                    periodic_wigner=True),
}
RATIO = (3.8, 4.2)      # second order: err(dt) / err(dt / 2)
EDGE = 1e-8             # the DVR state's Wigner function on the first and last row and column of the box, of its maximum
GPU_RICHARDSON, GPU_PLAIN = 4.0, 1.25  # margins of the device's figures over the restatements'
QUIRK_FACTOR = 100.0    # the driver's lengths put the dt = 0.01 state more than this many (c) bounds from the DVR answer


def coupled_case(name):
    """(num_pes, x, p, dx, dp, (x_first, dx, V, dV) on the grid) of a coupled case; max |p| stays inside the Wigner alias limit pi / (2 dx)
    (asserted in the host test)"""
    c = COUPLED[name]
    x, dx = box(c["n"], c["length"])
    p, dp = box(c["n"], c.get("p_length", c["length"]))
    return c["num_pes"], x, p, dx, dp, (x[0], dx, *quadratic_table(c["num_pes"], K_FORCE, c["A"], c["B"], x[0], dx, c["n"]))


def host_richardson(c, boundary):
    return c["richardson"][boundary]


def dvr_mass(boundary, n):
    """the mass to hand gple_dvr_hamiltonian for a particle of mass MASS.  The periodic kinetic matrix (general.cpp:106-200) is the Fourier
    one of period L = x[n - 1] - x[0] = (n - 1) dx, while the grid's period is n dx: every kinetic entry carries (n / (n - 1))^2, which is a
    mass of MASS ((n - 1) / n)^2.  Handing it MASS (n / (n - 1))^2 gives the operator of the grid's own period; without it the periodic run
    lies 4.2e-2 (n = 128) from the MQCLE and from the reflective run at every dt"""
    return MASS if boundary == REFLECTIVE else MASS * (n / (n - 1.0)) ** 2


def wigner_sum(c, boundary):
    """the boundary flag of gple_wigner for the chain on `boundary`.  The periodic sum takes psi(x - y) conj psi(x + y) with indices mod n for
    |y| <= n / 3 spacings: a state wider than a third of the box meets its own image there (on the boxes of 16: 2.5e-3 ... 3.8e-3 of the
    maximum from the sum without wrap-around, against 8.3e-10 on the box of 30), so only the wide box runs it; the others take the sum without wrap-around for both chains"""
    return PERIODIC if boundary == PERIODIC and c.get("periodic_wigner", False) else REFLECTIVE


def packet(num_pes, x):
    """the start of the coupled cases: the coherent packet of the k = mass = 1 oscillator on diabat 0"""
    psi = np.zeros(num_pes * len(x), dtype=complex)
    psi[:len(x)] = gaussian_state(x, PACKET_X0, 0.0, PACKET_SIGMA)
    return psi


def adiabatic_populations(psi_adia, num_pes, dx):
    return (np.abs(np.asarray(psi_adia).reshape(num_pes, -1)) ** 2).sum(axis=1) * dx


def diabatic_energies(V):
    """the `energies` argument of gple_wigner for diabatic amplitudes: V_aa(x), (n, N)"""
    return np.ascontiguousarray(np.einsum("iaa->ia", V))


def coupling_energy(W, V, dx, dp):
    """sum over a != b of the integral of W_ab V_ba: the averages of gple_wigner weigh the diagonal elements only (E_a(x) + p^2 / 2m on W_aa),
    which is the whole energy in a basis that diagonalises V; for diabatic amplitudes the couplings add this.  (The Wigner transform of the
    adiabatic amplitudes is no way round it: where the adiabatic states turn with x it is not the pointwise rotation of W that
    gple_mqcl_observe forms, and its (E, p) lie 4.5e-2 away on these cases.)"""
    N = W.shape[0]
    return sum(2.0 * (W[a, b].real * V[:, a, b][:, None]).sum() for a in range(N) for b in range(a + 1, N)) * dx * dp


def edge_fraction(W):
    """the largest element on the first and last row and column of the box over the largest anywhere; W (N, N, n_x, n_p)"""
    W = np.abs(W)
    return max(W[:, :, 0].max(), W[:, :, -1].max(), W[:, :, :, 0].max(), W[:, :, :, -1].max()) / W.max()


def scales(W, energies, x, p, mass, dx, dp):
    """the scale of (E, x, p) for a relative error of the state: the sums of the averages with every weight in absolute value, so a pointwise
    error of eps max |W| where the state lives moves an average by about eps times its scale, however the signed sum cancels"""
    density = sum(np.abs(W[a, a]) for a in range(W.shape[0])) * dx * dp
    e = np.abs(energies).max(axis=1)[:, None] + p[None, :] ** 2 / 2.0 / mass
    return np.array([(density * e).sum(), (density * np.abs(x)[:, None]).sum(), (density * np.abs(p)[None, :]).sum()])
