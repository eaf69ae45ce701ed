"""CPU: the numpy restatements of the trajectory methods (tests/hop_numpy.py, hop_mf_numpy.py, hop_sqc_numpy.py, hop_mash_numpy.py) against
references that are no restatement of their step (tests/hop_exact_cases.py; DESIGN.md §17, "Against closed forms and an ODE solution"):

  A  closed forms on V = k x^2 / 2 I + A + B x through a table: the harmonic flow and exp(-i A t) under constant coupling (A1), the displaced
     uncoupled parabolas from every start surface (A2); the float64 restatement lies within the recorded figures times HOST_MARGIN
  B  Tully's dual avoided crossing and the three-state model against a long double RK4 of the published equations: the reference converges
     with itself, the error of a restatement falls by 4 from dt = 1 to dt = 0.5, and at dt = 1 it is more than 100 bounds of the Richardson
     combination, so the comparison the GPU test makes sees the splitting
  C  the fewest-switches property: the fraction of an ensemble on each surface follows the mean |c_k|^2

The device is set against the same references in tests/test_gpu_hop_exact.py."""
import numpy as np
import pytest

from tests import hop_exact_cases as HX
from tests import hop_mash_numpy as HA
from tests import hop_numpy as HN

LD = np.longdouble


# ---- the references themselves -------------------------------------------------------------------------------------------------------------------
def test_the_closed_forms_stand_on_their_own():
    # exp(-i A t) by its series against the eigen-decomposition
    for A in HX.A1_A.values():
        t = HX.A_DT * HX.A_STEPS
        E, C = np.linalg.eigh(A)
        assert np.abs(HX.expm(-1j * A * t) - (C * np.exp(-1j * E * t)) @ C.T).max() < 1e-14
    # the powers of K D K are a rotation by theta per step, cos theta = 1 - k dt^2 / 2 m
    x0, p0, k, m, dt, K = LD(1.25), LD(-0.75), LD(1.5), LD(2), LD(0.05), 200
    path, p = HX.kdk_path(np.array([x0]), np.array([p0]), k, 0.0, m, dt, K)
    u, tau = k * dt * dt / (2 * m), dt / m
    c, s = 1 - u, np.sqrt(u * (2 - u))
    theta = np.arctan2(s, c)
    assert abs(path[-1, 0] - (x0 * np.cos(K * theta) + p0 * tau / s * np.sin(K * theta))) < 1e-17
    assert abs(p[0] - (p0 * np.cos(K * theta) - x0 * s / tau * np.sin(K * theta))) < 1e-17
    # a centre moves the flow with it
    moved, q = HX.kdk_path(np.array([x0 + 3]), np.array([p0]), k, 3.0, m, dt, K)
    assert np.abs(moved - 3 - path).max() < 1e-17 and abs(q[0] - p[0]) < 1e-17
    # A2: no two surfaces meet inside the box
    for N in (2, 3):
        assert (np.abs(HX.crossings(HX.A2_A[N], HX.A2_B[N])) > HX.A_BOX).all()
    assert np.abs(HX.crossings(np.diag([1.0, -1.0]), np.diag([0.5, -0.5]))).min() == 2.0  # and the condition can fail


def test_the_models_of_the_ode_are_the_library_s_and_their_derivatives_are_derivatives():
    x = np.linspace(-9.0, 9.0, 145).astype(LD)
    for model, num_pes, fun in HX.B_MODELS.values():
        V, dV = fun(x)
        Vr, Fr = HN.builtin(model, num_pes)(x)
        assert np.abs(V - Vr).max() < 1e-17 and np.abs(dV + Fr).max() < 1e-17  # products of constants formed in double there
        h = LD(2.0) ** -20
        up, down = fun(x + h)[0], fun(x - h)[0]
        third = np.abs(fun(x + 2 * h)[0] - 2 * up + 2 * down - fun(x - 2 * h)[0]).max() / 2  # h^3 V''': the central difference errs by a sixth of it
        assert np.abs((up - down) / (2 * h) - dV).max() < third / h + 1e-12
        assert np.array_equal(V, np.swapaxes(V, 1, 2)) and np.abs(dV).max() > 1e-3


# ---- A ---------------------------------------------------------------------------------------------------------------------------------------------
def check_a(name, group, ref):
    """the restatement within HOST_MARGIN recorded figures of the closed form; nobody left, nobody near a bound"""
    bound = HX.HOST_MARGIN * HX.A_HOST[group]
    print(f"hop exact host {name}: restatement - closed form x {ref['D'][0]:.3g} p {ref['D'][1]:.3g} b {ref['D'][2]:.3g} (bound {bound:.3g}); "
          f"least distance to a bound {ref['diag']['edge'].min():.3g}")
    assert (ref["end"][4] == 0).all() and ref["diag"]["edge"].min() > 1.0
    assert max(ref["D"]) <= bound, (name, ref["D"], bound)


@pytest.mark.parametrize("method,num_pes", HX.A1_METHODS)
def test_a1_constant_coupling(method, num_pes):
    start, ref = HX.a1_case(method, num_pes)
    norms = (np.abs(start[2]) ** 2).sum(axis=1)
    populations = np.abs(start[2]) ** 2
    assert populations.min(axis=1).max() > 0.2, "no true superposition"
    if method == "sqc":
        assert np.abs(norms - 1.0).max() > 0.1  # the spring constant differs from trajectory to trajectory
    else:
        assert np.abs(norms - 1.0).max() < 1e-14
    check_a(f"A1 {method} N = {num_pes}", f"A1 {method}", ref)
    if method in ("fssh", "mash"):
        assert np.array_equal(ref["end"][3], start[3]) and ref["diag"]["hops"].sum() == 0 and ref["diag"]["frustrated"].sum() == 0
    if method == "mash":
        _, potential = HX.a_table("A1", num_pes)
        c = HA.adiabatic(HN.states(start[0], potential)[2], start[2])
        assert np.abs(HA.norms(c)[:, 0] - HA.norms(c)[:, 1]).min() >= HX.MASH_MARGIN and ref["diag"]["margin"].min() >= HX.MASH_MARGIN


@pytest.mark.parametrize("num_pes,surface0", [(2, 0), (2, 1), (3, 0), (3, 1), (3, 2)])
def test_a2_displaced_uncoupled_surfaces(num_pes, surface0):
    for method in ("fssh", "mf"):
        start, ref = HX.a2_case(method, num_pes, surface0)
        d = ref["d"]
        assert d == np.argsort(np.diag(HX.A2_A[num_pes]))[surface0] and (np.abs(start[2][:, d]) == 1.0).all()
        check_a(f"A2 {method} N = {num_pes} from {surface0} (diabat {d})", "A2", ref)
        assert np.abs(np.abs(ref["end"][2][:, d]) - 1.0).max() <= HX.HOST_MARGIN * HX.A_HOST["A2"]
        assert np.count_nonzero(np.delete(ref["end"][2], d, axis=1)) == 0
        if method == "fssh":
            assert np.array_equal(ref["end"][3], start[3]) and ref["diag"]["hops"].sum() == 0 and ref["diag"]["frustrated"].sum() == 0
    # the surfaces differ: from another surface the trajectory ends elsewhere
    if surface0:
        assert np.abs(ref["want"][1] - HX.a2_case("mf", num_pes, 0)[1]["want"][1]).max() > 0.1


# ---- B ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,method", HX.B_RUNS)
def test_b_against_the_ode_solution(case, method):
    ref, fine = HX.b_reference(case, method), HX.b_reference(case, method, HX.B_H_FINE)
    own = HX.distance(ref, fine)
    recorded = HX.B_SELF_MEASURED[case, method]
    r = HX.b_restated(case, method)
    kept = int(r["keep"].sum())
    coarse, half, residual = HX.b_errors(case, method, r["runs"], r["keep"])
    bound = HX.b_bound(case, method, recorded)
    ratio = [a / b for a, b in zip(coarse, half)]
    print(f"hop exact host B {case} {method}: kept {kept} of {HX.B_N}; reference h = 1/8 against 1/16 " + " ".join(f"{v:.3g}" for v in own)
          + "; D " + " ".join(f"{v:.3g}" for v in r["D"]) + "; err(dt = 1) " + " ".join(f"{v:.3g}" for v in coarse)
          + "; ratio " + " ".join(f"{v:.5f}" for v in ratio) + "; Richardson residual " + " ".join(f"{v:.3g}" for v in residual)
          + "; bound " + " ".join(f"{v:.3g}" for v in bound))
    assert all(o <= s <= HX.B_SELF for o, s in zip(own, recorded)), (own, recorded)
    assert kept >= HX.B_KEEP and (kept == HX.B_N or method in ("fssh", "mash"))
    for q in range(3):
        assert HX.B_RATIO[0] <= ratio[q] <= HX.B_RATIO[1], (case, method, "xpb"[q], ratio[q])                 # (a)
        assert coarse[q] > HX.B_SEES * bound[q], (case, method, "xpb"[q], coarse[q], bound[q])                 # (c)
    # the force matters: without it the momentum would not have moved
    assert np.abs(ref[1] - r["start"][1]).max() > 1e-3


# ---- C ---------------------------------------------------------------------------------------------------------------------------------------------
def test_c_the_fraction_on_a_surface_follows_the_amplitudes():
    potential = HN.builtin(HN.DAC, 2)
    state = HN.sample(potential, 2, HX.C_N, HX.SEED, HX.B_X0, HX.C_P0, HX.C_SIGMA, HX.C_SIGMA, 0)
    worst, middle = 0.0, False
    for step in range(0, HX.C_LAST, HX.C_EVERY):
        state, _ = HN.evolve(potential, state, HX.SEED, HX.B_MASS, HX.C_DT, step, HX.C_EVERY, -HX.B_BOX, HX.B_BOX)
        x, _, b, surface, status = state
        assert (status == 0).all()
        c = np.einsum("mik,mi->mk", HN.states(x, potential)[2], b)
        for k in range(2):
            population, fraction = float((np.abs(c[:, k]) ** 2).mean()), float((surface == k).mean())
            sigma = max(np.sqrt(population * (1.0 - population) / HX.C_N), 1.0 / HX.C_N)
            worst = max(worst, abs(fraction - population) / sigma)
            middle |= 0.2 <= population <= 0.8
            assert abs(fraction - population) <= HX.C_SIGMAS * sigma, (step + HX.C_EVERY, k, fraction, population, sigma)
    print(f"hop exact host C: largest deviation {worst:.3g} sigma")
    assert middle, "the populations never moved"
