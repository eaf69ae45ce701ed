"""GPU: fewest-switches surface hopping (gple_hop_sample / _evolve / _observe, csrc/gple_hop.hip) against the numpy restatement
tests/hop_numpy.py, trajectory by trajectory.

Every ensemble has 293 trajectories (a tail that is no multiple of 64 or 256), x0 = -4, sigma_p = p0 / 20, bounds +-6, mass 2000.  Decisions
(surface, status, the number of hops) must be EQUAL; x, p and b lie within 64 D_q + 1e-13 max(1, max|q|), D_q being the largest distance
between the float64 and the long double restatement for that quantity and case, measured here.  A trajectory is set aside only where the
float64 restatement's own margin |xi - (g_1 + ... + g_k)| falls below 1e-10 at some step, and at most 1 % of a case may be.  The ratios
measured on the MI355X are in DESIGN.md §17."""
import ctypes as C
import functools

import numpy as np
import pytest

import gaussian_process_liouville_equation_amd as pkg
from gaussian_process_liouville_equation_amd import _capi, hopping, pes
from tests import hop_numpy as HN

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
N_TRAJ, X0, MASS, LEFT, RIGHT, SEED = 293, -4.0, 2000.0, -6.0, 6.0, 20250117
BAD_ARG = 1

# name: model (an id, or the built-in that is tabulated at dx = 1 / 16), levels, p0, dt, steps, start surface, GPLE_HOP_REVERSE
CASES = {
    "sac": dict(model=HN.SAC, N=2, p0=10.0, dt=2.0, steps=400),
    "dac16": dict(model=HN.DAC, N=2, p0=16.0, dt=1.0, steps=500),
    "dac30": dict(model=HN.DAC, N=2, p0=30.0, dt=1.0, steps=500),
    "dac10": dict(model=HN.DAC, N=2, p0=10.0, dt=2.0, steps=900),                       # frustrated hops, reflection
    "dac10-reverse": dict(model=HN.DAC, N=2, p0=10.0, dt=2.0, steps=900, reverse=True),
    "ecr": dict(model=HN.ECR, N=2, p0=10.0, dt=4.0, steps=700, surface0=1),             # from the upper surface: reflected through the coupling region
    "tsac": dict(model=HN.TSAC, N=3, p0=10.0, dt=4.0, steps=250, surface0=1),
    "table2": dict(model=HN.DAC, N=2, p0=16.0, dt=1.0, steps=500, tabulated=True),
    "table3": dict(model=HN.TSAC, N=3, p0=10.0, dt=4.0, steps=250, surface0=1, tabulated=True),
}
FRUSTRATED = ("dac10", "dac10-reverse")


def widen(state):
    x, p, b, surface, status = state
    return x.astype(np.longdouble), p.astype(np.longdouble), b.astype(np.clongdouble), surface, status


@functools.lru_cache(maxsize=None)
def tabulated(model, N):
    """pes.tabulate of a built-in model on [-8, 8] at dx = 1 / 16"""
    return HN.FunctionTable(*pes.tabulate(HN.scalar_function(HN.builtin(model, N)), -8.0, 1.0 / 16.0, 257))


@functools.lru_cache(maxsize=None)
def reference(name):
    """The case on the restatement, once: the float64 sample, its evolution in float64 (with diagnostics) and in long double, and D per quantity"""
    assert np.finfo(np.longdouble).eps < 1e-18  # or D calibrates nothing
    c = {"surface0": 0, "reverse": False, "tabulated": False, **CASES[name]}
    pot = HN.table(tabulated(c["model"], c["N"])) if c["tabulated"] else HN.builtin(c["model"], c["N"])
    start = HN.sample(pot, c["N"], N_TRAJ, SEED, X0, c["p0"], 1.0 / (2.0 * c["p0"] / 20.0), c["p0"] / 20.0, surface0=c["surface0"])
    end, diag = HN.evolve(pot, start, SEED, MASS, c["dt"], 0, c["steps"], LEFT, RIGHT, reverse=c["reverse"])
    wide, _ = HN.evolve(pot, widen(start), SEED, MASS, c["dt"], 0, c["steps"], LEFT, RIGHT, reverse=c["reverse"])
    assert np.array_equal(end[3], wide[3]) and np.array_equal(end[4], wide[4])
    D = [float(np.abs(end[q] - wide[q]).max()) for q in range(3)]
    return dict(case=c, potential=pot, start=start, end=end, diag=diag, D=D)


@pytest.fixture
def model_of(gpu):
    """model_of(case) -> the id on the session's context (a table is defined, and undefined when the test ends)"""
    ids = []

    def make(c):
        if not c["tabulated"]:
            return c["model"]
        t = tabulated(c["model"], c["N"])
        ids.append(gpu.pes_define(c["N"], t.x_first, t.dx, t.V, t.dV))
        return ids[-1]

    yield make
    for model in ids:
        gpu.pes_undefine(model)


def same_bits(a, b):
    return all(np.array_equal(u, v) and u.dtype == v.dtype for u, v in zip(a, b))


# ---- 1. parity per trajectory ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_parity_per_trajectory(gpu, model_of, name):
    ref = reference(name)
    c, diag, (Dx, Dp, Db) = ref["case"], ref["diag"], ref["D"]
    model = model_of(c)
    evolve = lambda state, first, steps: gpu.hop_evolve(c["N"], model, state, SEED, MASS, c["dt"], first, steps, LEFT, RIGHT, reverse=c["reverse"])
    got = evolve(ref["start"], 0, c["steps"])  # one launch: the state never leaves the registers
    # the number of hops of every trajectory, from the same steps taken one launch each; by the way the same bits
    state, hops = ref["start"], np.zeros(N_TRAJ, dtype=np.int64)
    for s in range(c["steps"]):
        nxt = evolve(state, s, 1)
        hops += nxt[3] != state[3]
        state = nxt
    assert same_bits(state, got)
    assert diag["hops"].sum() >= 10, "the case tests nothing"
    if name in FRUSTRATED:
        assert diag["frustrated"].sum() >= 10, "the case tests nothing"
    keep = diag["margin"] >= 1e-10
    assert (~keep).sum() <= N_TRAJ // 100
    want = ref["end"]
    tol = [HN.tolerance(D, want[q]) for q, D in enumerate((Dx, Dp, Db))]
    err = [float(np.abs(got[q] - want[q])[keep].max()) for q in range(3)]
    print(f"hop parity {name}: hops {diag['hops'].sum()} frustrated {diag['frustrated'].sum()} least margin {diag['margin'].min():.3g} set aside {(~keep).sum()}; "
          f"D x {Dx:.3g} p {Dp:.3g} b {Db:.3g}; err / tol x {err[0] / tol[0]:.3g} p {err[1] / tol[1]:.3g} b {err[2] / tol[2]:.3g}; "
          f"least |r| / p^2 {diag['ratio'].min():.3g}, least distance to a bound {diag['edge'].min():.3g}")
    assert np.array_equal(got[3][keep], want[3][keep]) and np.array_equal(got[4][keep], want[4][keep]) and np.array_equal(hops[keep], diag["hops"][keep])
    for q in range(3):
        assert err[q] <= tol[q], (name, "xpb"[q], err[q], tol[q])


# ---- 2. bits ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dac10", "table3"])
def test_bits(gpu, model_of, name):
    import torch

    ref = reference(name)
    c, start = ref["case"], ref["start"]
    model = model_of(c)
    evolve = lambda state, first, steps, **kw: gpu.hop_evolve(c["N"], model, state, SEED, MASS, c["dt"], first, steps, LEFT, RIGHT, reverse=c["reverse"], **kw)
    steps, cut = 400, 150
    whole = evolve(start, 0, steps)
    assert same_bits(evolve(evolve(start, 0, cut), cut, steps - cut), whole)           # nothing hidden between two calls
    assert same_bits(evolve(start, 0, steps), whole)                                     # a repeat
    part = evolve(tuple(a[100:] for a in start), 0, steps, trajectory_offset=100)       # a slice with its offset
    assert same_bits(part, tuple(a[100:] for a in whole))
    where = torch.device("cuda", gpu.device)                                             # device pointers
    on_device = tuple(torch.from_numpy(a.copy()).to(where) for a in start)
    torch.cuda.synchronize(where)
    out = evolve(on_device, 0, steps)
    gpu.synchronize()
    assert all(o is d for o, d in zip(out, on_device))
    assert same_bits(tuple(t.cpu().numpy() for t in out), whole)
    done = whole[4] != 0                                                                 # a finished trajectory is frozen
    assert done.any()
    later = evolve(whole, steps, 200)
    assert same_bits(tuple(a[done] for a in later), tuple(a[done] for a in whole))
    other = gpu.hop_evolve(c["N"], model, start, SEED + 1, MASS, c["dt"], 0, steps, LEFT, RIGHT, reverse=c["reverse"])  # another seed, other hops
    assert (other[3] != whole[3]).any() and not np.array_equal(other[1], whole[1])


# ---- 3. sample ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,surface0", [("dac16", 0), ("tsac", 2), ("table2", 1)])
def test_sample(gpu, model_of, name, surface0):
    ref = reference(name)
    c, pot = ref["case"], ref["potential"]
    model = model_of(c)
    sx, sp = 1.0 / (2.0 * c["p0"] / 20.0), c["p0"] / 20.0
    x, p, b, surface, status = gpu.hop_sample(c["N"], model, N_TRAJ, SEED, X0, c["p0"], sx, sp, surface0)
    xr, pr, _, _, _ = HN.sample(pot, c["N"], N_TRAJ, SEED, X0, c["p0"], sx, sp, surface0)
    ex, ep = np.abs(x - xr).max() / (8 * EPS * (abs(X0) + 6 * sx)), np.abs(p - pr).max() / (8 * EPS * (abs(c["p0"]) + 6 * sp))
    print(f"hop sample {name}: err / tol x {ex:.3g} p {ep:.3g}")
    assert ex <= 1.0 and ep <= 1.0
    assert (surface == surface0).all() and (status == 0).all() and (b.imag == 0).all()
    assert np.abs(np.sum(b.real ** 2, axis=1) - 1.0).max() <= 8 * EPS
    _, _, Cm, _ = HN.states(x, pot)  # the adiabatic states at the device's own x
    c_adia = np.abs(np.einsum("mik,mi->mk", Cm, b.real))
    assert np.abs(c_adia - np.eye(c["N"])[surface0]).max() <= 1e-13
    # a slice with its offset, device pointers, a repeat: the same bits
    part = gpu.hop_sample(c["N"], model, 93, SEED, X0, c["p0"], sx, sp, surface0, trajectory_offset=200)
    assert same_bits(part, tuple(a[200:] for a in (x, p, b, surface, status)))
    dev = gpu.hop_sample(c["N"], model, N_TRAJ, SEED, X0, c["p0"], sx, sp, surface0, device_out=True)
    assert same_bits(tuple(t.cpu().numpy() for t in dev), (x, p, b, surface, status))


# ---- 4. observe ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dac10", "tsac", "table3"])
def test_observe(gpu, model_of, name):
    import torch

    ref = reference(name)
    c, state = ref["case"], ref["end"]
    model = model_of(c)
    N = c["N"]
    out = gpu.hop_observe(N, model, state, MASS)
    terms = HN.observe_terms(ref["potential"], state, MASS)
    assert out.shape == (4 * N + 3,)
    assert np.array_equal(out[:3 * N], terms[:, :3 * N].sum(axis=0)) and out[:3 * N].sum() == N_TRAJ
    assert out[:3 * N].reshape(3, N)[1:].sum() > 0  # some have left
    bound = N_TRAJ * EPS * np.abs(terms[:, 3 * N:]).sum(axis=0)
    err = np.abs(out[3 * N:] - terms[:, 3 * N:].sum(axis=0))
    print(f"hop observe {name}: err / tol {np.max(err / bound):.3g}")
    assert (err <= bound).all()
    assert np.array_equal(gpu.hop_observe(N, model, state, MASS), out)
    where = torch.device("cuda", gpu.device)
    on_device = tuple(torch.from_numpy(a.copy()).to(where) for a in state)
    torch.cuda.synchronize(where)
    assert np.array_equal(gpu.hop_observe(N, model, on_device, MASS), out)


# ---- 5. GPLE_ERR_BAD_ARG ------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments(gpu):
    ref = reference("dac16")
    lib, ctx = gpu.lib, gpu.ctx
    x, p, b, surface, status = (a.copy() for a in ref["start"])
    before = tuple(a.copy() for a in (x, p, b, surface, status))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    arrays = dict(x=x.ctypes.data_as(dp), p=p.ctypes.data_as(dp), b=b.ctypes.data_as(dp), surface=surface.ctypes.data_as(ip), status=status.ctypes.data_as(ip))
    out = np.zeros(11)
    nan, inf = float("nan"), float("inf")

    def sample(**kw):
        a = dict(num_pes=2, model=1, n=N_TRAJ, offset=0, seed=1, x0=X0, p0=16.0, sigma_x=0.625, sigma_p=0.8, surface0=0, flags=0, **arrays)
        a.update(kw)
        return lib.gple_hop_sample(ctx, a["num_pes"], a["model"], a["n"], a["offset"], a["seed"], a["x0"], a["p0"], a["sigma_x"], a["sigma_p"], a["surface0"], a["flags"],
                                   a["x"], a["p"], a["b"], a["surface"], a["status"])

    def evolve(**kw):
        a = dict(num_pes=2, model=1, n=N_TRAJ, offset=0, seed=1, mass=MASS, dt=1.0, first=0, steps=3, left=LEFT, right=RIGHT, flags=0, **arrays)
        a.update(kw)
        return lib.gple_hop_evolve(ctx, a["num_pes"], a["model"], a["n"], a["offset"], a["seed"], a["mass"], a["dt"], a["first"], a["steps"], a["left"], a["right"],
                                   a["flags"], a["x"], a["p"], a["b"], a["surface"], a["status"])

    def observe(**kw):
        a = dict(num_pes=2, model=1, n=N_TRAJ, mass=MASS, flags=0, out=out.ctypes.data_as(dp), **arrays)
        a.update(kw)
        return lib.gple_hop_observe(ctx, a["num_pes"], a["model"], a["n"], a["mass"], a["flags"], a["x"], a["p"], a["b"], a["surface"], a["status"], a["out"])

    table = tabulated(HN.DAC, 2)
    mine = gpu.pes_define(2, table.x_first, table.dx, table.V, table.dV)
    other = pkg.open_api(0)
    try:
        theirs = other.pes_define(2, table.x_first, table.dx, table.V, table.dV)
        theirs = other.pes_define(2, table.x_first, table.dx, table.V, table.dV)  # a second slot, free on the session's context
        assert theirs != mine
        shared = [dict(num_pes=1), dict(num_pes=4), dict(model=-1), dict(model=3), dict(model=7), dict(model=_capi.PES_USER + 15), dict(model=theirs),
                  dict(model=mine, num_pes=3), dict(n=0)]
        for kw in shared + [dict(offset=(1 << 32) - N_TRAJ + 1), dict(sigma_x=0.0), dict(sigma_x=-1.0), dict(sigma_x=nan), dict(sigma_x=inf), dict(sigma_p=0.0),
                            dict(sigma_p=nan), dict(sigma_p=inf), dict(surface0=-1), dict(surface0=2)] + [{k: None} for k in arrays]:
            assert sample(**kw) == BAD_ARG, kw
        for kw in shared + [dict(offset=(1 << 32) - N_TRAJ + 1), dict(mass=0.0), dict(mass=-1.0), dict(mass=nan), dict(mass=inf), dict(dt=0.0), dict(dt=-1.0),
                            dict(dt=nan), dict(dt=inf), dict(left=RIGHT), dict(left=7.0), dict(left=nan), dict(right=nan)] + [{k: None} for k in arrays]:
            assert evolve(**kw) == BAD_ARG, kw
        for kw in shared + [dict(mass=0.0), dict(mass=nan), dict(mass=inf), dict(out=None)] + [{k: None} for k in arrays]:
            assert observe(**kw) == BAD_ARG, kw
        assert same_bits((x, p, b, surface, status), before) and not out.any()  # a refused call writes nothing
        # what is not refused: the last admissible offset, the user model, no step at all
        assert evolve(offset=(1 << 32) - N_TRAJ) == 0 and evolve(model=mine) == 0 and observe(model=mine) == 0
        x, p, b, surface, status = (a.copy() for a in before)
        assert evolve(steps=0, x=x.ctypes.data_as(dp)) == 0 and np.array_equal(x, before[0])
    finally:
        other.close()
        gpu.pes_undefine(mine)


# ---- 6. the driver ------------------------------------------------------------------------------------------------------------------------------
def test_driver_against_the_same_loop_on_the_restatement(gpu, tmp_path):
    kw = dict(model=hopping.DAC, num_pes=2, ln_energy=-2.0, n_traj=512, seed=SEED, dt=2.0, x0=X0, xmin=LEFT, xmax=RIGHT)
    res = hopping.run(gpu, out_dir=str(tmp_path), **kw)
    narrow = hopping.run(HN.NumpyHopApi(), **kw)
    wide = hopping.run(HN.NumpyHopApi(dtype=np.longdouble), **kw)
    assert res["stop"] is not None and res["stop"] == narrow["stop"] == wide["stop"] and len(res["records"]) == len(narrow["records"]) == len(wide["records"]) > 10
    assert hasattr(res["state"][0], "is_cuda") and res["state"][0].is_cuda  # the ensemble stayed on the device
    worst = {}
    for key in ("x", "p", "E", "populations"):
        got, f64, ld = (np.array([r[key] for r in run["records"]]) for run in (res, narrow, wide))
        tol = HN.tolerance(np.abs(f64 - ld).max(), f64)
        worst[key] = np.abs(got - f64).max() / tol
    print("hop driver: %d outputs; err / tol %s" % (len(res["records"]), ", ".join(f"{k} {v:.3g}" for k, v in worst.items())))
    for a, b in zip(res["records"], narrow["records"]):
        assert a["t"] == b["t"] and np.array_equal(a["counts"], b["counts"])
    assert all(v <= 1.0 for v in worst.values()), worst
    assert sum(r["counts"][:, 1].sum() for r in res["records"]) > 0  # somebody hopped
    line = [float(v) for v in res["scattering_line"].split()]
    assert res["scattering_line"] == narrow["scattering_line"] and len(line) == 6 and abs(sum(line[1:]) - 1.0) < 1e-5 and line[-1] == 0.0
    t = [float(l) for l in open(tmp_path / "t.txt")]
    av = [[float(v) for v in l.split()] for l in open(tmp_path / "averages.txt")]
    assert len(t) == len(av) == len(res["records"])
    for rec, tt, row in zip(res["records"], t, av):
        want = [rec["t"], rec["E"], rec["x"], rec["p"], *(rec["counts"].sum(axis=0) / 512), *rec["populations"]]
        assert np.allclose([tt] + row, [rec["t"]] + want, rtol=1e-5, atol=1e-300)
