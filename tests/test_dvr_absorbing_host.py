"""CPU: the absorbing boundary of the exact DVR dynamics — the set-up of exact.setup(boundary=ABSORBING), the absorber, P4 and the binary power
of the restatement (tests/dvr_absorbing_numpy.py) against long-double RK4 stepping, and the driver exact.run on a numpy stand-in for the api."""
import math

import numpy as np
import pytest

from gaussian_process_liouville_equation_amd import exact
from tests import dvr_absorbing_numpy as AN
from tests import dvr_numpy as DN

EPS = np.finfo(np.float64).eps


# ---- set-up -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ln_e, n_abs, n, log2_dt, halvings", [(0, 7, 1935, -6, 0), (1, 9, 3859, -8, 6), (2, 11, 7703, -9, 13), (3, 13, 15387, -10, 3)])
def test_setup_at_the_absorbing_defaults(ln_e, n_abs, n, log2_dt, halvings):
    s = exact.setup(float(ln_e), boundary=exact.ABSORBING)
    assert (s["n_absorbing"], s["n_grids"], s["dt_rule"], s["halvings"]) == (n_abs, n, 2.0 ** log2_dt, halvings)
    assert s["dt"] == s["dt_rule"] / 2 ** halvings
    p0, sp = s["p0"], s["sigma_p"]
    assert s["absorbing_length"] == 2 * math.pi / (p0 - 3 * sp)
    # main.cpp:108: the box edges are grid points, the absorbing points lie outside them and stop short of the pole
    assert s["x"][n_abs] == -15.0 and s["x"][n - 1 - n_abs] == 15.0 and np.array_equal(s["x"], -15.0 + s["dx"] * (np.arange(n) - n_abs))
    assert -15.0 - s["x"][0] < s["absorbing_length"] and s["x"][-1] - 15.0 < s["absorbing_length"]
    # main.cpp:134, 144-145 with the counts doubled per halving: the output times are those of the reference's dt
    assert s["output_step"] == int(s["output_time"] / s["dt_rule"]) * 2 ** halvings and s["total_step"] == int(s["total_time"] / s["dt_rule"]) * 2 ** halvings
    assert s["output_step"] * s["dt"] == int(s["output_time"] / s["dt_rule"]) * s["dt_rule"]
    # the halving rule: the absorber's term inside RK4's real-axis interval, and not halved once more than needed
    w = AN.absorber(s["x"], s["mass"], -15.0, 15.0, s["absorbing_length"])
    assert s["dt"] * w.max() <= 2.0 and (halvings == 0 or 2 * s["dt"] * w.max() > 2.0)
    assert s["w_max"] == pytest.approx(w.max(), rel=1e-13)
    # the kinetic rule of main.cpp:134 keeps dt |T| <= 0.64 (the Colbert-Miller spectrum ends at (pi hbar / dx)^2 / 2 m)
    assert s["dt_rule"] * (math.pi / s["dx"]) ** 2 / 2 / s["mass"] <= 0.64


def test_rk4_stability_rectangle():
    """[-2.5, 0] x [-0.7, 0.7] lies inside RK4's stability region |P4(z)| <= 1: what the halving rule (real part) and the kinetic rule (imaginary
    part) rely on, sampled at a spacing of 1e-3"""
    re, im = np.meshgrid(np.linspace(-2.5, 0.0, 2501), np.linspace(-0.7, 0.7, 1401))
    z = re + 1j * im
    P = 1 + z * (1 + z / 2 * (1 + z / 3 * (1 + z / 4)))
    assert np.abs(P).max() <= 1.0 + 1e-15
    inner = (re < -0.02)
    assert np.abs(P)[inner].max() < 1.0


def _old_setup(ln_energy=0.0, mass=2000.0, x0=-8.0, xmin=-15.0, xmax=15.0, dx_max=0.1, number_of_output=50):
    """main.cpp:52-146 without an absorbing region, written out again"""
    p0 = float(np.sqrt(2.0 * mass * np.exp(ln_energy)))
    sigma_p = p0 / 20.0
    output_time = float(exact.output_time_cutoff((-x0 - x0) / (p0 / mass) / number_of_output))
    dx = exact.cutoff(min(dx_max, 2 * math.pi / (p0 + 3.0 * sigma_p) / 5.0))
    n = int((xmax - xmin) / dx) + 1
    pmin, pmax = p0 - math.pi / dx / 2.0, p0 + math.pi / dx / 2.0
    i = np.arange(n)
    total_time = (xmax - xmin) / (p0 / mass) * 2.0
    return dict(mass=mass, x0=x0, p0=p0, sigma_p=sigma_p, sigma_x=1.0 / 2.0 / sigma_p, xmin=xmin, xmax=xmax, dx=dx, n_grids=n, x=xmin + dx * i,
                p=((n - 1 - i) * pmin + i * pmax) / (n - 1), total_time=total_time, output_time=output_time, dt=output_time,
                total_step=int(total_time / output_time), output_step=1)


@pytest.mark.parametrize("ln_e", [-4.0, 0.0, 1.0])
def test_other_boundaries_are_unchanged(ln_e):
    old = _old_setup(ln_e)
    for s in (exact.setup(ln_e), exact.setup(ln_e, boundary=exact.REFLECTIVE), exact.setup(ln_e, boundary=exact.PERIODIC, dt_max=0.01)):
        assert sorted(s) == sorted(old)
        for k, v in old.items():
            assert np.array_equal(np.asarray(s[k]), np.asarray(v)) and type(s[k]) is type(v), k
    assert (exact.REFLECTIVE, exact.PERIODIC, exact.ABSORBING) == (0, 1, 2)


# ---- the absorber -----------------------------------------------------------------------------------------------------------------------------
def test_absorber_properties():
    assert abs(AN.C_ABS - 2.6220575542921198) <= 4 * EPS
    for s in (exact.setup(0.0, boundary=exact.ABSORBING), exact.setup(-1.0, boundary=exact.ABSORBING, dx=0.125)):
        x, n, na, L = s["x"], s["n_grids"], s["n_absorbing"], s["absorbing_length"]
        w = AN.absorber(x, s["mass"], s["xmin"], s["xmax"], L)
        assert (w >= 0.0).all()
        assert not w[na:n - na].any() and (w[:na] > 0).all() and (w[n - na:] > 0).all()  # exactly 0 inside the box and at both edges
        assert np.abs(w - w[::-1]).max() <= 64 * EPS * w.max()  # mirror symmetric (the grid is, up to the rounding of xmin + dx a)
        assert (np.diff(w[:na + 1]) < 0).all() and (np.diff(w[n - na - 1:]) > 0).all()  # rising monotonically towards the pole
        # the driver's own host copy (it sizes dt with it) is the same function
        assert np.abs(exact.absorbing_potential(x, s["mass"], s["xmin"], s["xmax"], L) - w).max() <= 8 * EPS * w.max()
        # the reference's literal branch (pes.cpp:91, `x < xmin`) at the grid point x == xmin: a gain — the defect the library does not restate
        lit = AN.absorber(x, s["mass"], s["xmin"], s["xmax"], L, literal=True)
        assert x[na] == s["xmin"] and lit[na] < 0.0 and w[na] == 0.0
        assert np.array_equal(np.delete(lit, na), np.delete(w, na))


# ---- P4 and the powers ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_pes, n", AN.SHAPES)
def test_p4_is_a_contraction_after_the_halving_rule(num_pes, n):
    c = AN.case(num_pes, n)
    P = AN.p4(AN.generator(c["H"], c["W"], num_pes, c["dt"]))
    assert np.linalg.norm(P, 2) <= 1.0 + 1e-12
    assert np.abs(P - P.T).max() <= 8 * EPS  # complex symmetric
    # one application is one RK4 step
    one = AN.rk4_states(c["H"], c["W"], num_pes, c["dt"], c["psi0"], (1,))[1]
    assert np.linalg.norm((P @ c["psi0"]).astype(np.clongdouble) - one) <= 8 * EPS * math.sqrt(c["dim"]) * np.linalg.norm(c["psi0"])


@pytest.mark.parametrize("num_pes, n, s", [(2, 37, 37), (2, 23, 1000), (3, 43, 3), (2, 96, 2)])
def test_binary_power_against_long_double_stepping(num_pes, n, s):
    """First-order error analysis: P4 is a contraction (above), so a perturbation of P of relative size dim eps (one rounded product) moves
    P^s by at most s times that, and each of the <= 2 log2 s products of the power adds dim eps of its own, doubled by every later squaring:
    s dim eps |psi0| bounds the sum.  (dim 74, s = 37: 6e-13 |psi0| allowed.)"""
    c = AN.case(num_pes, n)
    err = AN.reference_error(num_pes, n, s)
    assert err <= s * c["dim"] * EPS * np.linalg.norm(c["psi0"]), err / np.linalg.norm(c["psi0"])
    # the norm never grows along the stepping
    norms = [np.linalg.norm(c["psi0"])] + [float(np.linalg.norm(c["states"][k])) for k in AN.POWERS]
    assert (np.diff(norms) <= 0).all()


# ---- the driver on a numpy stand-in -----------------------------------------------------------------------------------------------------------
SMALL = dict(AN.SMALL, output_time=64.0)


class NumpyApi:
    """the restatement behind the entry points exact.run calls (no format_g: the Python writer); script: states handed out instead of U psi"""

    def __init__(self, script=None):
        self.script, self.calls = script, []

    def dvr_hamiltonian(self, num_pes, model, boundary, x_first, dx, n, mass):
        from oracle import evolve_oracle_n as ON
        self.calls.append(("hamiltonian", boundary))
        E, Cb, _, _ = ON.adiabatic(DN.grid(x_first, dx, n), model, num_pes)
        return DN.hamiltonian(num_pes, model, boundary, x_first, dx, n, mass), E, Cb

    def dvr_absorber(self, x_first, dx, n, mass, xmin, xmax, length):
        return AN.absorber(DN.grid(x_first, dx, n), mass, xmin, xmax, length)

    def dvr_propagator(self, num_pes, n, H, W, dt, n_steps, device_out=False):
        self.calls.append(("propagator", n_steps, dt))
        return AN.power(AN.p4(AN.generator(H, W, num_pes, dt)), n_steps)

    def dvr_apply(self, num_pes, n, U, psi0, T, basis=None):
        self.calls.append(("apply", T))
        out = np.empty((T, len(psi0)), dtype=np.complex128)
        for k in range(T):
            psi0 = out[k] = self.script.pop(0) if self.script is not None else U @ psi0
        return out

    def dvr_propagate(self, *a, **k):
        raise AssertionError("the absorbing run does not propagate spectrally")

    def wigner(self, num_pes, boundary, x_first, dx, p, psi, energies=None, mass=0.0, phase=True, averages=False):
        self.calls.append(("wigner", boundary))
        P = np.stack([DN.wigner(v, num_pes, boundary, dx, p, dtype=np.complex128)[0] for v in psi])
        x = DN.grid(x_first, dx, psi.shape[1] // num_pes)
        return (P if phase else None), np.stack([DN.wigner_averages(Pt, x, p, energies, mass, dx) for Pt in P])


def test_driver_files_and_records(tmp_path):
    api = NumpyApi()
    res = exact.run(api, model=exact.SAC, num_pes=2, boundary=exact.ABSORBING, out_dir=str(tmp_path), write_phase="text", max_outputs=4, chunk_bytes=1_600_000,
                    **SMALL)
    s = res["setup"]
    assert (s["n_grids"], s["n_absorbing"], s["dt"], s["halvings"], s["output_step"]) == (107, 5, 0.125, 0, 512)
    # no eigh and no spectral propagation; H and the Wigner transform of the reflective boundary; one propagator, applied in chunks
    assert res["eigh_seconds"] == 0.0
    assert [c for c in api.calls if c[0] in ("hamiltonian", "wigner")] == [("hamiltonian", 0)] + [("wigner", 0)] * 2
    assert [c for c in api.calls if c[0] == "propagator"] == [("propagator", 512, 0.125)]
    assert [c for c in api.calls if c[0] == "apply"] == [("apply", 1), ("apply", 2)]  # psi0 is the first output; chunks of two
    from oracle import evolve_oracle_n as ON
    ref, _ = AN.run_loop(s, 2, exact.SAC, 4, ON.adiabatic(s["x"], exact.SAC, 2)[1])
    assert len(res["records"]) == len(ref) == 4
    for a, b in zip(res["records"], ref):
        assert a["t"] == b["t"]
        assert np.abs(a["populations"] - b["populations"]).max() <= 1e-12
        assert abs(a["E"] - b["E"]) <= 1e-12 * abs(b["E"]) and abs(a["x"] - b["x"]) <= 1e-12
    assert [r["t"] for r in res["records"]] == [0.0, 64.0, 128.0, 192.0]
    for name, lines in (("x.txt", 107), ("p.txt", 107), ("t.txt", 4), ("psi.txt", 4), ("averages.txt", 4)):
        assert len(open(tmp_path / name).read().splitlines()) == lines, name
    assert len(open(tmp_path / "phase.txt").read().split("\n")) == 5 * 4 + 1
    assert [float(v) for v in open(tmp_path / "x.txt").read().split()] == [float("%g" % v) for v in s["x"]]
    row = [float(v) for v in open(tmp_path / "averages.txt").read().splitlines()[2].split()]
    assert len(row) == 9 and row[0] == 128.0 and row[4:6] == [float("%g" % v) for v in ref[2]["populations"]]
    assert res["stop"] is None and len(res["final_line"].split()) == 3 and res["final_line"].split()[0] == "20"


def _packet(s, centre, weight):
    """a Gaussian of total population `weight` around `centre` on the lower diabatic surface"""
    g = DN.gaussian(s["x"], centre, s["p0"], 0.2) * math.sqrt(weight)
    return np.concatenate([g, np.zeros_like(g)])


STOPS = [
    ("GET OUT OF INTERACTING REGION", [(-1.0, 1.0), (0.5, 0.95), (1.8, 0.9)], 4),
    ("DIRECTION REVERSED DUE TO REFLECTION / PBC", [(0.5, 0.9), (0.4, 1e-6)], 3),        # reversed outranks absorbed
    ("ALMOST ALL POPULATION HAVE BEEN ABSORBED", [(-0.5, 1e-5), (0.5, 1e-5)], 3),         # absorbed outranks stable
    ("ALMOST ALL POPULATION HAVE BEEN ABSORBED", [(0.5, 1.5e-4), (0.9, 0.99e-4)], 3),     # <x> = sum x |psi|^2 dx is not normalised: it must still grow
    ("POPULATION ON EACH PES IS STABLE", [(0.5, 2e-4), (0.5, 2e-4 + 5e-6)], 3),          # above PplLim, change below ChangeLim
    (None, [(-1.0, 1.0), (0.5, 0.9), (0.6, 0.8), (0.7, 0.7)], 5),                         # nothing fires: the outputs run out
]


@pytest.mark.parametrize("message, script, n_records", STOPS)
def test_every_stop_branch(message, script, n_records):
    s = exact.setup(boundary=exact.ABSORBING, **SMALL)
    api = NumpyApi([_packet(s, c, w) for c, w in script])
    said = []
    res = exact.run(api, model=exact.SAC, num_pes=2, boundary=exact.ABSORBING, write_phase=None, max_outputs=len(script) + 1, log=said.append, **SMALL)
    assert len(res["records"]) == n_records
    if message is None:
        assert res["stop"] is None and said[-1] == "FINISHED ALL OUTPUT TIMES"
    else:
        assert res["stop"] == f"{message}, STOP EVOLVING AT {res['stop_time']:g}" or res["stop"] == f"{message}. STOP EVOLVING AT {res['stop_time']:g}"
        assert said[-1] == res["stop"]


def test_non_absorbing_runs_never_say_absorbed():
    """the PplLim clause belongs to the absorbing boundary alone (main.cpp:269)"""
    s = exact.setup(**SMALL)

    class Spectral(NumpyApi):
        def dvr_propagate(self, num_pes, n, eigvec, eigval, psi0, times):
            return np.stack([_packet(s, 0.5, 5e-5), _packet(s, 0.5, 9e-5)][:len(times)])

    res = exact.run(Spectral(), model=exact.SAC, num_pes=2, boundary=exact.REFLECTIVE, write_phase=None, max_outputs=2, **SMALL)
    assert res["stop"] is None and len(res["records"]) == 2
