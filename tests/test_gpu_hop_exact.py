"""GPU: the trajectory kernels of csrc/gple_hop.hip (gple_hop_evolve, _evolve_mf, _evolve_sqc, _evolve_mash) against references that are no
restatement of their step (tests/hop_exact_cases.py; DESIGN.md §17, "Against closed forms and an ODE solution").

  A  closed forms on V = k x^2 / 2 I + A + B x, registered as a table (gple_pes_define): 293 trajectories, 200 steps of dt = 0.05, bounds +-6.
     The device lies within 64 D_q + 1e-13 max(1, max|q|) of the long double closed form, D_q being the distance of the float64 restatement
     from that closed form for the case and quantity, computed here; surfaces and statuses are equal.
  B  Tully's dual avoided crossing and the three-state model against a long double RK4 of the published equations, 32 trajectories, at dt = 1
     and dt = 0.5: the error falls by a factor in [3.8, 4.2], and the Richardson combination lies within twice the float64 restatement's
     own residual plus the tolerance above (D_q now the distance between the float64 and the long double restatement) plus the reference's
     self-convergence figure.  Fewest switches and MASH are compared on the trajectories that the restatement keeps on their surface.

Every ensemble starts from the restatement's sample (MASH in part A from gple_hop_sample_mash), so the references and the device integrate the
same initial values.  The figures measured on the MI355X are in DESIGN.md §17; tests/test_hop_exact_host.py holds the CPU side."""
import numpy as np
import pytest

from tests import hop_exact_cases as HX
from tests import hop_mash_numpy as HA
from tests import hop_numpy as HN

pytestmark = pytest.mark.gpu


def device(gpu, method, num_pes, model, state, mass, dt, steps, left, right):
    """the method's kernel on a numpy ensemble -> the evolved copy"""
    if method == "fssh":
        return gpu.hop_evolve(num_pes, model, state, HX.SEED, mass, dt, 0, steps, left, right)
    if method == "mf":
        return gpu.hop_evolve_mf(num_pes, model, state, mass, dt, steps, left, right)
    if method == "sqc":
        return gpu.hop_evolve_sqc(num_pes, model, state, mass, dt, steps, left, right, HX.GAMMA)
    return gpu.hop_evolve_mash(num_pes, model, state, mass, dt, steps, left, right)


@pytest.fixture
def table_of(gpu):
    """table_of(which, num_pes) -> the id of the part A table on the session's context, undefined when the test ends"""
    ids = []

    def make(which, num_pes):
        ids.append(gpu.pes_define(num_pes, *HX.a_table(which, num_pes)[0]))
        return ids[-1]

    yield make
    for model in ids:
        gpu.pes_undefine(model)


def check_a(name, got, ref):
    """the device within tolerance(D_q, q) of the closed form, per quantity"""
    want, D = ref["want"], ref["D"]
    err = HX.distance(got, want)
    tol = [HN.tolerance(D[q], want[q]) for q in range(3)]
    print(f"hop exact {name}: D x {D[0]:.3g} p {D[1]:.3g} b {D[2]:.3g}; err x {err[0]:.3g} p {err[1]:.3g} b {err[2]:.3g}; "
          f"err / tol x {err[0] / tol[0]:.3g} p {err[1] / tol[1]:.3g} b {err[2] / tol[2]:.3g}")
    assert (got[4] == 0).all()
    for q in range(3):
        assert err[q] <= tol[q], (name, "xpb"[q], err[q], tol[q])


# ---- A1 ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,num_pes", HX.A1_METHODS)
def test_a1_constant_coupling(gpu, table_of, method, num_pes):
    model = table_of("A1", num_pes)
    if method == "mash":
        start = gpu.hop_sample_mash(num_pes, model, HX.A_N, HX.SEED, HX.A1_X0, 0.0, HX.A_SIGMA, HX.A_SIGMA, 0)
        c = HA.adiabatic(HN.states(start[0], HX.a_table("A1", num_pes)[1])[2], start[2])
        assert np.abs(HA.norms(c)[:, 0] - HA.norms(c)[:, 1]).min() >= HX.MASH_MARGIN
        ref = HX.a1_reference(method, num_pes, start)
        assert ref["diag"]["margin"].min() >= HX.MASH_MARGIN
    else:
        start, ref = HX.a1_case(method, num_pes)
    got = device(gpu, method, num_pes, model, start, HX.A_MASS, HX.A_DT, HX.A_STEPS, -HX.A_BOX, HX.A_BOX)
    check_a(f"A1 {method} N = {num_pes}", got, ref)
    if method in ("fssh", "mash"):
        assert np.array_equal(got[3], start[3])


# ---- A2 ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_pes,surface0", [(2, 0), (2, 1), (3, 0), (3, 1), (3, 2)])
def test_a2_displaced_uncoupled_surfaces(gpu, table_of, num_pes, surface0):
    model = table_of("A2", num_pes)
    for method in ("fssh", "mf"):
        start, ref = HX.a2_case(method, num_pes, surface0)
        got = device(gpu, method, num_pes, model, start, HX.A_MASS, HX.A_DT, HX.A_STEPS, -HX.A_BOX, HX.A_BOX)
        check_a(f"A2 {method} N = {num_pes} from {surface0} (diabat {ref['d']})", got, ref)
        off = np.abs(np.abs(got[2][:, ref["d"]]) - 1.0).max()
        print(f"hop exact A2 {method} N = {num_pes} from {surface0}: | |b_d| - 1 | {off:.3g}")
        assert off <= HN.tolerance(ref["D"][2], ref["want"][2])
        if method == "fssh":
            assert np.array_equal(got[3], start[3])  # no hop


# ---- B -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,method", HX.B_RUNS)
def test_b_against_the_ode_solution(gpu, case, method):
    c = HX.B_CASES[case]
    model, num_pes, _ = HX.B_MODELS[c["model"]]
    r = HX.b_restated(case, method)
    keep = r["keep"]
    assert keep.sum() >= HX.B_KEEP
    runs = [device(gpu, method, num_pes, model, r["start"], HX.B_MASS, dt, int(round(c["T"] / dt)), -HX.B_BOX, HX.B_BOX) for dt in HX.B_DTS]
    for got, want in zip(runs, r["runs"]):  # the device decides as the restatement does
        assert np.array_equal(got[4], want[4])
        if method in ("fssh", "mash"):
            assert np.array_equal(got[3][keep], want[3][keep])
    coarse, half, residual = HX.b_errors(case, method, runs, keep)
    bound = HX.b_bound(case, method, HX.B_SELF_MEASURED[case, method])
    ratio = [a / b for a, b in zip(coarse, half)]
    print(f"hop exact B {case} {method}: kept {keep.sum()} of {HX.B_N}; D " + " ".join(f"{v:.3g}" for v in r["D"])
          + "; err(dt = 1) " + " ".join(f"{v:.3g}" for v in coarse) + "; ratio " + " ".join(f"{v:.5f}" for v in ratio)
          + "; Richardson residual " + " ".join(f"{v:.3g}" for v in residual) + "; residual / bound " + " ".join(f"{a / b:.3g}" for a, b in zip(residual, bound)))
    for q in range(3):
        assert HX.B_RATIO[0] <= ratio[q] <= HX.B_RATIO[1], (case, method, "xpb"[q], ratio[q])   # (a)
        assert residual[q] <= bound[q], (case, method, "xpb"[q], residual[q], bound[q])         # (b)
