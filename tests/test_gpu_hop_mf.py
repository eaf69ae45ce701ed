"""GPU: Ehrenfest (mean-field) trajectories (gple_hop_evolve_mf / _observe_mf and their _groups forms, csrc/gple_hop.hip; DESIGN.md §17,
"Mean-field (Ehrenfest) trajectories") against the numpy restatement tests/hop_mf_numpy.py, trajectory by trajectory, against themselves bit
for bit, and against the fewest-switches kernel where the two must agree.

Every ensemble is the sample of tests/test_gpu_hop.py: 293 trajectories (a tail that is no multiple of 64 or 256), x0 = -4, sigma_p = p0 / 20,
sigma_x = 1 / (2 sigma_p), bounds +-6, mass 2000, seed 20250117.  The status must be EQUAL for every trajectory; x, p and b lie within
64 D_q + 1e-13 max(1, max|q|), D_q being the largest distance between the float64 and the long double restatement for that quantity and case,
computed here.  No trajectory is set aside: the only decision of the step is the bound, and the restatement shows that no trajectory of any
case comes closer to one than 1e-9.  The sums of observe lie within n eps sum|term| of the restatement's, except in the one column where the
float64 restatement misses its own long double evaluation by more than that (TSAC's closed top channel on the left, sum 2.8e-15: 10.7 times
the bound, 25.6 for the table; the device is 12.9 and 31.1 times the bound from the float64 restatement there); test_observe says what
holds in that column.  The ratios measured on the MI355X are in DESIGN.md §17."""
import ctypes as C
import functools

import numpy as np
import pytest

from gaussian_process_liouville_equation_amd import _capi, hopping, pes
from tests import hop_mf_numpy as HM
from tests import hop_numpy as HN
from tests import hop_scan_numpy as HS

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
N_TRAJ, X0, MASS, LEFT, RIGHT, SEED = 293, -4.0, 2000.0, -6.0, 6.0, 20250117
BAD_ARG = 1

# name: model (an id, or the built-in that is tabulated at dx = 1 / 16), levels, p0, dt, steps, start surface
CASES = {
    "sac": dict(model=HN.SAC, N=2, p0=10.0, dt=2.0, steps=400),
    "dac16": dict(model=HN.DAC, N=2, p0=16.0, dt=1.0, steps=1500),
    "dac10": dict(model=HN.DAC, N=2, p0=10.0, dt=2.0, steps=900),
    "ecr": dict(model=HN.ECR, N=2, p0=10.0, dt=4.0, steps=700, surface0=1),
    "tsac": dict(model=HN.TSAC, N=3, p0=10.0, dt=4.0, steps=600, surface0=0),
    "table2": dict(model=HN.DAC, N=2, p0=10.0, dt=2.0, steps=900, tabulated=True),
    "table3": dict(model=HN.TSAC, N=3, p0=10.0, dt=4.0, steps=600, surface0=0, tabulated=True),
}
MIXED = ("dac10", "tsac", "table3")  # at least 10 trajectories in each of at least two statuses


def decoupled(x):
    """two levels that never meet and never couple: a step and, 0.05 above it, a bump"""
    V = np.array([[0.003 * np.tanh(x), 0.0], [0.0, 0.06 + 0.01 * np.exp(-0.5 * x * x)]])
    dV = np.array([[0.003 / np.cosh(x) ** 2, 0.0], [0.0, -0.01 * x * np.exp(-0.5 * x * x)]])
    return V, dV


def widen(state):
    x, p, b, surface, status = state
    return x.astype(np.longdouble), p.astype(np.longdouble), b.astype(np.clongdouble), surface, status


@functools.lru_cache(maxsize=None)
def tabulated(model, N):
    """pes.tabulate of a built-in model on [-8, 8] at dx = 1 / 16; model None: the decoupled pair"""
    fun = decoupled if model is None else HN.scalar_function(HN.builtin(model, N))
    return HN.FunctionTable(*pes.tabulate(fun, -8.0, 1.0 / 16.0, 257))


@functools.lru_cache(maxsize=None)
def reference(name):
    """The case on the restatement, once: the float64 sample, its evolution in float64 (with diagnostics) and in long double, and D per quantity"""
    assert np.finfo(np.longdouble).eps < 1e-18  # or D calibrates nothing
    if name == "decoupled":
        c = dict(model=None, N=2, p0=10.0, dt=2.0, steps=1100, surface0=0, tabulated=True)
    else:
        c = {"surface0": 0, "tabulated": False, **CASES[name]}
    pot = HN.table(tabulated(c["model"], c["N"])) if c["tabulated"] else HN.builtin(c["model"], c["N"])
    start = HN.sample(pot, c["N"], N_TRAJ, SEED, X0, c["p0"], 1.0 / (2.0 * c["p0"] / 20.0), c["p0"] / 20.0, surface0=c["surface0"])
    end, diag = HM.evolve(pot, start, MASS, c["dt"], c["steps"], LEFT, RIGHT)
    wide, _ = HM.evolve(pot, widen(start), MASS, c["dt"], c["steps"], LEFT, RIGHT)
    assert np.array_equal(end[4], wide[4])
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


def physical(state):
    """x, p, b, status: what a mean-field call reads and writes"""
    return tuple(state[q] for q in (0, 1, 2, 4))


def on_device(gpu, *arrays):
    import torch

    where = torch.device("cuda", gpu.device)
    out = tuple(torch.from_numpy(np.ascontiguousarray(a).copy()).to(where) for a in arrays)
    torch.cuda.synchronize(where)
    return out


# ---- 1. parity per trajectory ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_parity_per_trajectory(gpu, model_of, name):
    ref = reference(name)
    c, diag, D, want = ref["case"], ref["diag"], ref["D"], ref["end"]
    per_status = np.bincount(want[4], minlength=3)
    assert diag["edge"].min() >= 1e-9, "a trajectory of the restatement decides its bound within rounding: change the case"
    if name in MIXED:
        assert (per_status >= 10).sum() >= 2, "the case tests nothing"
    got = gpu.hop_evolve_mf(c["N"], model_of(c), ref["start"], MASS, c["dt"], c["steps"], LEFT, RIGHT)  # one launch: the state never leaves the registers
    tol = [HN.tolerance(D[q], want[q]) for q in range(3)]
    err = [float(np.abs(got[q] - want[q]).max()) for q in range(3)]
    print(f"mean field parity {name}: running / left / right {per_status}, least distance to a bound {diag['edge'].min():.3g}; D x {D[0]:.3g} p {D[1]:.3g} "
          f"b {D[2]:.3g}; err / tol x {err[0] / tol[0]:.3g} p {err[1] / tol[1]:.3g} b {err[2] / tol[2]:.3g}")
    assert np.array_equal(got[4], want[4]) and got[4].dtype == np.int32
    assert got[3] is ref["start"][3]
    for q in range(3):
        assert err[q] <= tol[q], (name, "xpb"[q], err[q], tol[q])
    assert np.abs(np.sum(HM.norms(got[2]), axis=1) - 1.0).max() <= 1e-12


# ---- 2. observe ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dac10", "tsac", "table3"])
def test_observe(gpu, model_of, name):
    ref = reference(name)
    c, state = ref["case"], ref["end"]
    model, N = model_of(c), c["N"]
    out = gpu.hop_observe_mf(N, model, state, MASS)
    terms = HM.observe_terms(ref["potential"], state, MASS)
    assert out.shape == (3 * N + 6,)
    counts = out[3 * N:3 * N + 3]
    assert np.array_equal(counts, np.bincount(state[4], minlength=3)) and counts.sum() == N_TRAJ and (counts > 0).sum() >= 2
    bound = N_TRAJ * EPS * np.abs(terms).sum(axis=0)
    err = np.abs(out - terms.sum(axis=0))
    # The rule n eps sum|term| bounds the error of ADDING terms that both sides form alike.  It cannot be met where the float64 reference misses
    # its own long double evaluation by more than that: the weight of a closed channel (TSAC's top state on the left: 2.8e-15 over six
    # trajectories, |c_k| = 2e-8), whose terms are squares of a cancellation residue of C^T b, good to eps / |c_k| in any float64 arithmetic.
    # Such a column is found from the reference alone, never from the device, and gets 64 times the reference's own error on top, the
    # project's rule for a rounding floor (HN.tolerance); every other column is held to the rule as it stands
    own = np.abs(terms.sum(axis=0) - HM.observe_terms(ref["potential"], widen(state), MASS).sum(axis=0)).astype(np.float64)
    sound = own <= bound
    slack = np.where(sound, 0.0, 64.0 * own)
    ratio = np.divide(err, bound, out=np.zeros_like(err), where=bound > 0)
    print(f"mean field observe {name}: err / tol {ratio[sound].max():.3g}; columns the float64 reference cannot arbitrate {np.nonzero(~sound)[0].tolist()}: "
          f"reference's own error / tol {(own[~sound] / bound[~sound]).round(1).tolist()}, device err / tol {ratio[~sound].round(1).tolist()}")
    assert (~sound).sum() <= 1 and (np.abs(terms).sum(axis=0)[~sound] < 1e-12).all()
    assert (err <= bound + slack).all()
    assert np.array_equal(gpu.hop_observe_mf(N, model, state, MASS), out)
    assert np.array_equal(gpu.hop_observe_mf(N, model, on_device(gpu, *state), MASS), out)
    odd = state[:4] + (np.where(np.arange(N_TRAJ) % 50 == 0, np.where(np.arange(N_TRAJ) % 100 == 0, 3, -1), state[4]).astype(np.int32),)
    skipped = gpu.hop_observe_mf(N, model, odd, MASS)  # a status out of range: no weight, no count; x, p and the energy as before
    assert np.array_equal(skipped[3 * N:3 * N + 3], np.bincount(odd[4][(odd[4] >= 0) & (odd[4] <= 2)], minlength=3)) and skipped[3 * N:3 * N + 3].sum() == N_TRAJ - 6
    assert np.array_equal(skipped[3 * N + 3:], out[3 * N + 3:]) and abs(skipped[:3 * N].sum() - (N_TRAJ - 6)) < 1e-10


# ---- 3. bits ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dac10", "table3"])
def test_bits(gpu, model_of, name):
    ref = reference(name)
    c, start = ref["case"], ref["start"]
    model = model_of(c)
    evolve = lambda state, steps: gpu.hop_evolve_mf(c["N"], model, state, MASS, c["dt"], steps, LEFT, RIGHT)
    steps, cut = c["steps"], c["steps"] // 3
    whole = evolve(start, steps)
    assert same_bits(evolve(evolve(start, cut), steps - cut), whole)                     # nothing hidden between two calls
    assert same_bits(evolve(start, steps), whole)                                        # a repeat
    assert same_bits(evolve(tuple(a[100:] for a in start), steps), tuple(a[100:] for a in whole))  # a slice
    dev = on_device(gpu, *start)                                                         # device pointers
    out = evolve(dev, steps)
    gpu.synchronize()
    assert all(o is d for o, d in zip(out, dev))
    assert same_bits(tuple(t.cpu().numpy() for t in out), whole)
    done = whole[4] != 0                                                                 # a finished trajectory is frozen
    assert done.sum() >= 10 and (~done).sum() >= 10
    later = evolve(whole, 200)
    assert same_bits(tuple(a[done] for a in later), tuple(a[done] for a in whole)) and not np.array_equal(later[0][~done], whole[0][~done])
    marked = (start[0], start[1], start[2], np.arange(N_TRAJ, dtype=np.int32) - 7, start[4])  # the surface is never read and never written
    assert same_bits(physical(evolve(marked, steps)), physical(whole)) and evolve(marked, steps)[3] is marked[3]
    assert np.array_equal(marked[3], np.arange(N_TRAJ, dtype=np.int32) - 7)
    surface = on_device(gpu, marked[3])[0]
    dev = on_device(gpu, *start)
    out = evolve(dev[:3] + (surface,) + dev[4:], steps)
    gpu.synchronize()
    assert out[3] is surface and np.array_equal(surface.cpu().numpy(), marked[3])


# ---- 4. groups ----------------------------------------------------------------------------------------------------------------------------------
GROUPS = {"5x67": dict(N=2, model=HN.DAC, tabulated=False, p0=[8.0, 10.0, 16.0, 24.0, 30.0], dt=[2.0, 2.0, 1.0, 1.0, 0.5], steps=1500),
          "130x1": dict(N=3, model=HN.TSAC, tabulated=True, p0=list(np.linspace(8.0, 14.0, 130)), dt=list(np.where(np.arange(130) % 3 == 0, 4.0, 2.0)), steps=800),
          "2x300": dict(N=2, model=HN.DAC, tabulated=False, p0=[10.0, 24.0], dt=[2.0, 1.0], steps=800)}


@pytest.mark.parametrize("shape", list(GROUPS))
def test_groups_are_the_plain_calls_on_slices(gpu, model_of, shape):
    c = GROUPS[shape]
    n_groups, n_per = (int(v) for v in shape.split("x"))
    model, N, steps, dt = model_of(c), c["N"], c["steps"], np.array(c["dt"])
    p0 = np.array(c["p0"])
    packets = np.stack([np.full(n_groups, X0), p0, 1.0 / (2.0 * p0 / 20.0), p0 / 20.0], axis=1)
    start = gpu.hop_sample_groups(N, model, n_per, SEED, packets, 0)
    grouped = lambda state, table, count: gpu.hop_evolve_groups_mf(N, model, state, n_per, MASS, table, count, LEFT, RIGHT)
    equal = np.full(n_groups, 2.0)                                                        # one dt for all: the plain call over the whole
    whole = gpu.hop_evolve_mf(N, model, start, MASS, 2.0, steps, LEFT, RIGHT)
    same = grouped(start, equal, steps)
    assert same_bits(same, whole)
    for sl in HS.slices(n_groups, n_per)[:5]:                                             # ... which is the plain call per slice
        assert same_bits(gpu.hop_evolve_mf(N, model, tuple(a[sl] for a in start), MASS, 2.0, steps, LEFT, RIGHT), tuple(a[sl] for a in whole))
    mixed = grouped(start, dt, steps)                                                      # differing dt: one plain call per group
    assert same_bits(grouped(grouped(start, dt, 150), dt, steps - 150), mixed) and mixed[3] is start[3]
    rows = gpu.hop_observe_groups_mf(N, model, mixed, n_per, MASS)
    assert rows.shape == (n_groups, 3 * N + 6) and np.array_equal(gpu.hop_observe_groups_mf(N, model, mixed, n_per, MASS), rows)
    assert (rows[:, 3 * N:3 * N + 3].sum(axis=1) == n_per).all()
    for g, sl in enumerate(HS.slices(n_groups, n_per)):
        plain = gpu.hop_evolve_mf(N, model, tuple(a[sl] for a in start), MASS, dt[g], steps, LEFT, RIGHT)
        assert same_bits(plain, tuple(a[sl] for a in mixed)), g
        assert np.array_equal(gpu.hop_observe_mf(N, model, plain, MASS), rows[g]), g
    dev = on_device(gpu, *start)                                                           # device pointers
    out = grouped(dev, dt, steps)
    gpu.synchronize()
    assert all(o is d for o, d in zip(out, dev)) and same_bits(tuple(t.cpu().numpy() for t in out), mixed)
    assert np.array_equal(gpu.hop_observe_groups_mf(N, model, out, n_per, MASS), rows)
    done = mixed[4] != 0
    print(f"mean field groups {shape}: finished {done.sum()} of {len(done)}")
    assert done.any() and (~done).any(), "the case tests nothing"


# ---- 5. against the fewest-switches kernel --------------------------------------------------------------------------------------------------------
def test_decoupled_levels_follow_the_active_surface(gpu, model_of):
    """Two levels that never couple: Fd is diagonal and b stays on its level, so the mean-field force is the force of that level (to the
    rounding of |b_0|^2), and gple_hop_evolve never hops (F_ak is exactly 0): both kernels integrate the same trajectory"""
    ref = reference("decoupled")
    c, start = ref["case"], ref["start"]
    model = model_of(c)
    assert (start[2][:, 1] == 0).all() and (np.abs(start[2][:, 0]) == 1).all()
    mf = gpu.hop_evolve_mf(2, model, start, MASS, c["dt"], c["steps"], LEFT, RIGHT)
    tully = gpu.hop_evolve(2, model, start, SEED, MASS, c["dt"], 0, c["steps"], LEFT, RIGHT)
    assert (tully[3] == 0).all() and np.array_equal(mf[4], tully[4]) and np.array_equal(mf[4], ref["end"][4])
    tol = [HN.tolerance(ref["D"][q], ref["end"][q]) for q in range(2)]
    err = [float(np.abs(mf[q] - tully[q]).max()) for q in range(2)]
    print(f"mean field against fewest switches: running / left / right {np.bincount(mf[4], minlength=3)}; err / tol x {err[0] / tol[0]:.3g} p {err[1] / tol[1]:.3g}")
    assert err[0] <= tol[0] and err[1] <= tol[1]
    assert (mf[4] != 0).sum() >= 10


# ---- 6. GPLE_ERR_BAD_ARG --------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments(gpu):
    ref = reference("dac16")
    lib, ctx = gpu.lib, gpu.ctx
    x, p, b, _, status = (a.copy() for a in ref["start"])
    n_groups, n_per = 1, N_TRAJ
    out, rows = np.full(12, -1.0), np.full((1, 12), -1.0)
    before = tuple(a.copy() for a in (x, p, b, status, out, rows))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    arrays = dict(x=x.ctypes.data_as(dp), p=p.ctypes.data_as(dp), b=b.ctypes.data_as(dp), status=status.ctypes.data_as(ip))
    nan, inf = float("nan"), float("inf")
    tables = []  # keeps the tables of the calls alive

    def table(values):
        tables.append(np.ascontiguousarray(values, dtype=np.float64))
        return tables[-1].ctypes.data_as(dp)

    def evolve(**kw):
        a = dict(num_pes=2, model=1, n=N_TRAJ, mass=MASS, dt=1.0, steps=3, left=LEFT, right=RIGHT, flags=0, **arrays)
        a.update(kw)
        return lib.gple_hop_evolve_mf(ctx, a["num_pes"], a["model"], a["n"], a["mass"], a["dt"], a["steps"], a["left"], a["right"], a["flags"], a["x"], a["p"],
                                      a["b"], a["status"])

    def evolve_groups(**kw):
        a = dict(num_pes=2, model=1, groups=n_groups, per=n_per, mass=MASS, dt=table([1.0]), steps=3, left=LEFT, right=RIGHT, flags=0, **arrays)
        a.update(kw)
        return lib.gple_hop_evolve_groups_mf(ctx, a["num_pes"], a["model"], a["groups"], a["per"], a["mass"], a["dt"], a["steps"], a["left"], a["right"], a["flags"],
                                             a["x"], a["p"], a["b"], a["status"])

    def observe(**kw):
        a = dict(num_pes=2, model=1, n=N_TRAJ, mass=MASS, flags=0, out=out.ctypes.data_as(dp), **arrays)
        a.update(kw)
        return lib.gple_hop_observe_mf(ctx, a["num_pes"], a["model"], a["n"], a["mass"], a["flags"], a["x"], a["p"], a["b"], a["status"], a["out"])

    def observe_groups(**kw):
        a = dict(num_pes=2, model=1, groups=n_groups, per=n_per, mass=MASS, flags=0, out=rows.ctypes.data_as(dp), **arrays)
        a.update(kw)
        return lib.gple_hop_observe_groups_mf(ctx, a["num_pes"], a["model"], a["groups"], a["per"], a["mass"], a["flags"], a["x"], a["p"], a["b"], a["status"],
                                              a["out"])

    t = tabulated(HN.DAC, 2)
    mine = gpu.pes_define(2, t.x_first, t.dx, t.V, t.dV)
    try:
        models = [dict(num_pes=1), dict(num_pes=4), dict(model=-1), dict(model=3), dict(model=7), dict(model=_capi.PES_USER + 15), dict(model=mine, num_pes=3)]
        nulls = [{k: None} for k in arrays]
        sizes = [dict(n=0), dict(n=(1 << 32) + 1)]
        group_sizes = [dict(groups=0), dict(per=0), dict(groups=_capi.HOP_MAX_GROUPS + 1, per=1), dict(groups=65536, per=1 << 60),
                       dict(groups=5, per=(1 << 64) // 5 + 1), dict(groups=4, per=(1 << 30) + 1)]
        stepping = [dict(mass=0.0), dict(mass=-1.0), dict(mass=nan), dict(mass=inf), dict(left=RIGHT), dict(left=7.0), dict(left=nan), dict(right=nan),
                    dict(right=inf), dict(steps=(1 << 40) + 1), dict(flags=_capi.HOP_REVERSE)]
        for kw in models + nulls + sizes + stepping + [dict(dt=0.0), dict(dt=-1.0), dict(dt=nan), dict(dt=inf)]:
            assert evolve(**kw) == BAD_ARG, kw
        for kw in models + nulls + group_sizes + stepping + [dict(dt=None)] + [dict(dt=table([v])) for v in (0.0, -1.0, nan, inf)]:
            assert evolve_groups(**kw) == BAD_ARG, kw
        assert evolve_groups(groups=2, per=100, dt=table([1.0, nan])) == BAD_ARG and evolve_groups(groups=2, per=100, dt=table([-1.0, 1.0])) == BAD_ARG
        for kw in models + nulls + sizes + [dict(mass=0.0), dict(mass=nan), dict(mass=inf), dict(out=None)]:
            assert observe(**kw) == BAD_ARG, kw
        for kw in models + nulls + group_sizes + [dict(mass=0.0), dict(mass=nan), dict(mass=inf), dict(out=None)]:
            assert observe_groups(**kw) == BAD_ARG, kw
        assert same_bits((x, p, b, status, out, rows), before)  # a refused call writes nothing
        # what is not refused: the user model, no step at all, the longest admissible call of no steps
        assert evolve(steps=0) == 0 and evolve_groups(steps=0) == 0 and same_bits((x, p, b, status), before[:4])
        assert observe(model=mine) == 0 and observe_groups(model=mine) == 0 and np.array_equal(out, rows[0]) and out[6:9].sum() == N_TRAJ
        assert evolve(model=mine) == 0 and not np.array_equal(x, before[0])
    finally:
        gpu.pes_undefine(mine)


# ---- 7. the driver --------------------------------------------------------------------------------------------------------------------------------
def test_driver_against_the_same_loop_on_the_restatement(gpu, tmp_path):
    kw = dict(model=hopping.DAC, num_pes=2, ln_energy=-2.0, n_traj=512, seed=SEED, dt=2.0, x0=X0, xmin=LEFT, xmax=RIGHT, method="ehrenfest")
    res = hopping.run(gpu, out_dir=str(tmp_path), **kw)
    narrow = hopping.run(HM.NumpyMfApi(), **kw)
    wide = hopping.run(HM.NumpyMfApi(dtype=np.longdouble), **kw)
    assert res["stop"] is not None and res["stop"] == narrow["stop"] == wide["stop"] and len(res["records"]) == len(narrow["records"]) == len(wide["records"]) > 10
    assert hasattr(res["state"][0], "is_cuda") and res["state"][0].is_cuda  # the ensemble stayed on the device
    worst = {}
    for key in ("x", "p", "E", "populations", "weights"):
        got, f64, ld = (np.array([r[key] for r in run["records"]]) for run in (res, narrow, wide))
        if key == "weights":
            got, f64, ld = got / 512, f64 / 512, ld / 512
        tol = HN.tolerance(np.abs(f64 - ld).max(), f64)
        worst[key] = np.abs(got - f64).max() / tol
    print("mean field driver: %d outputs; err / tol %s" % (len(res["records"]), ", ".join(f"{k} {v:.3g}" for k, v in worst.items())))
    for a, b in zip(res["records"], narrow["records"]):
        assert a["t"] == b["t"] and np.array_equal(a["n_status"], b["n_status"])
    assert all(v <= 1.0 for v in worst.values()), worst
    line = [float(v) for v in res["scattering_line"].split()]
    assert len(line) == 6 and abs(sum(line[1:]) - 1.0) < 1e-5 and line[-1] == 0.0 and min(line[3], line[4]) > 0.0
    assert np.allclose(line, [float(v) for v in narrow["scattering_line"].split()], rtol=1e-5, atol=1e-6)
    t = [float(l) for l in open(tmp_path / "t.txt")]
    av = [[float(v) for v in l.split()] for l in open(tmp_path / "averages.txt")]
    assert len(t) == len(av) == len(res["records"])
    for rec, tt, row in zip(res["records"], t, av):
        assert np.allclose([tt] + row, [rec["t"], rec["t"], rec["E"], rec["x"], rec["p"], *rec["populations"]], rtol=1e-5, atol=1e-300)
