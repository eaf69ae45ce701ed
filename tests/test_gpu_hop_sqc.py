"""GPU: symmetrical quasi-classical trajectories (gple_hop_sample_sqc / _evolve_sqc / _observe_sqc and their _groups forms, csrc/gple_hop.hip;
DESIGN.md §17, "Symmetrical quasi-classical trajectories") against the numpy restatement tests/hop_sqc_numpy.py, trajectory by trajectory, against
themselves bit for bit, and against the mean-field kernel at gamma = 0.

Every ensemble is the sample of tests/test_gpu_hop.py: 293 trajectories (a tail that is no multiple of 64 or 256), x0 = -4, sigma_p = p0 / 20,
sigma_x = 1 / (2 sigma_p), bounds +-6, mass 2000, seed 20250117; every case runs with both windows at their customary gamma.  The status and the
window index, at the start and at the end, must be EQUAL for every trajectory; x, p and b (the sample's b too) lie within
64 D_q + 1e-13 max(1, max|q|), D_q being the largest distance between the float64 and the long double restatement for that quantity and case,
computed here.  No trajectory is set aside.  Instead two margins are asserted on the restatement alone: no x_new comes within 1e-9 of a bound,
and no e comes within 1e-9 of a window edge it is compared with, at the start or at the end.  The device's window index of a trajectory is read
from gple_hop_observe_groups_sqc with groups of one.  The figures measured on the MI355X are in DESIGN.md §17."""
import ctypes as C
import functools

import numpy as np
import pytest

from gaussian_process_liouville_equation_amd import _capi, hopping, pes
from tests import hop_mf_numpy as HM
from tests import hop_numpy as HN
from tests import hop_scan_numpy as HS
from tests import hop_sqc_numpy as HQ

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
N_TRAJ, X0, MASS, LEFT, RIGHT, SEED = 293, -4.0, 2000.0, -6.0, 6.0, 20250117
BAD_ARG = 1
WINDOWS = {"square": HQ.SQUARE, "triangle": HQ.TRIANGLE}

# name: model (an id, or the built-in that is tabulated at dx = 1 / 16), levels, p0, dt, steps, start surface
CASES = {
    "sac": dict(model=HN.SAC, N=2, p0=10.0, dt=2.0, steps=400),
    "dac16": dict(model=HN.DAC, N=2, p0=16.0, dt=1.0, steps=1500),
    "dac10": dict(model=HN.DAC, N=2, p0=10.0, dt=2.0, steps=900),
    "ecr": dict(model=HN.ECR, N=2, p0=10.0, dt=4.0, steps=700, surface0=1),
    "tsac0": dict(model=HN.TSAC, N=3, p0=10.0, dt=4.0, steps=600, surface0=0),
    "tsac1": dict(model=HN.TSAC, N=3, p0=10.0, dt=4.0, steps=600, surface0=1),
    "table2": dict(model=HN.DAC, N=2, p0=10.0, dt=2.0, steps=900, tabulated=True),
    "table3": dict(model=HN.TSAC, N=3, p0=10.0, dt=4.0, steps=600, surface0=0, tabulated=True),
}
BOTH = [(name, window) for name in CASES for window in WINDOWS]


def widen(state):
    x, p, b, surface, status = state
    return x.astype(np.longdouble), p.astype(np.longdouble), b.astype(np.clongdouble), surface, status


@functools.lru_cache(maxsize=None)
def tabulated(model, N):
    """pes.tabulate of a built-in model on [-8, 8] at dx = 1 / 16"""
    return HN.FunctionTable(*pes.tabulate(HN.scalar_function(HN.builtin(model, N)), -8.0, 1.0 / 16.0, 257))


def packet(p0):
    return X0, p0, 1.0 / (2.0 * p0 / 20.0), p0 / 20.0


@functools.lru_cache(maxsize=None)
def reference(name, window):
    """The case on the restatement, once: the float64 sample (and D of its b), its evolution in float64 (with diagnostics) and in long double, D
    per quantity, the window index and the margin of every trajectory at the start and at the end"""
    assert np.finfo(np.longdouble).eps < 1e-18  # or D calibrates nothing
    c = {"surface0": 0, "tabulated": False, **CASES[name]}
    code = WINDOWS[window]
    gamma = HQ.GAMMA[code]
    pot = HN.table(tabulated(c["model"], c["N"])) if c["tabulated"] else HN.builtin(c["model"], c["N"])
    start = HQ.sample(pot, c["N"], N_TRAJ, SEED, *packet(c["p0"]), c["surface0"], code, gamma)
    wide_start = HQ.sample(pot, c["N"], N_TRAJ, SEED, *packet(c["p0"]), c["surface0"], code, gamma, dtype=np.longdouble)
    end, diag = HQ.evolve(pot, start, MASS, c["dt"], c["steps"], LEFT, RIGHT, gamma, drift=False)
    wide, _ = HQ.evolve(pot, widen(start), MASS, c["dt"], c["steps"], LEFT, RIGHT, gamma, drift=False)
    assert np.array_equal(end[4], wide[4])
    D = [float(np.abs(end[q] - wide[q]).max()) for q in range(3)]
    e_start, e_end = HQ.energies(pot, start)[0], HQ.energies(pot, end)[0]
    return dict(case=c, potential=pot, window=code, gamma=gamma, start=start, end=end, diag=diag, D=D, D_sample=float(np.abs(start[2] - wide_start[2]).max()),
                window_start=HQ.window_of(e_start, code, gamma), window_end=HQ.window_of(e_end, code, gamma),
                margin=min(HQ.margin(e_start, code, gamma).min(), HQ.margin(e_end, code, gamma).min()))


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
    """x, p, b, status: what an evolve or observe call reads and writes"""
    return tuple(state[q] for q in (0, 1, 2, 4))


def on_device(gpu, *arrays):
    import torch

    where = torch.device("cuda", gpu.device)
    out = tuple(torch.from_numpy(np.ascontiguousarray(a).copy()).to(where) for a in arrays)
    torch.cuda.synchronize(where)
    return out


def device_windows(gpu, N, model, state, code, gamma):
    """the window index (-1: none) the device gives every trajectory: its row of the grouped sums with groups of one"""
    rows = gpu.hop_observe_groups_sqc(N, model, state, 1, MASS, code, gamma)
    cells = rows[:, :3 * N].reshape(-1, 3, N).sum(axis=1)
    none = rows[:, 3 * N + 3:3 * N + 6].sum(axis=1)
    assert np.array_equal(cells.sum(axis=1) + none, np.ones(len(rows)))
    return np.where(none == 1, -1, np.argmax(cells, axis=1))


# ---- 1. the sample ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,window", BOTH)
def test_sample(gpu, model_of, name, window):
    ref = reference(name, window)
    c, code, gamma, want = ref["case"], ref["window"], ref["gamma"], ref["start"]
    model, N = model_of(c), c["N"]
    got = gpu.hop_sample_sqc(N, model, N_TRAJ, SEED, *packet(c["p0"]), c["surface0"], code, gamma)
    plain = gpu.hop_sample(N, model, N_TRAJ, SEED, *packet(c["p0"]), c["surface0"])
    assert same_bits((got[0], got[1], got[3], got[4]), (plain[0], plain[1], plain[3], plain[4]))  # x and p have the bits of gple_hop_sample
    assert (got[3] == c["surface0"]).all() and (got[4] == 0).all()
    tol, err = HN.tolerance(ref["D_sample"], want[2]), float(np.abs(got[2] - want[2]).max())
    print(f"sqc sample {name} {window}: D b {ref['D_sample']:.3g}; err / tol b {err / tol:.3g}; least window margin {ref['margin']:.3g}")
    assert ref["margin"] >= 1e-9, "an e of the restatement decides its window within rounding: change the case"
    assert err <= tol and (ref["window_start"] == c["surface0"]).all()
    assert np.array_equal(device_windows(gpu, N, model, got, code, gamma), ref["window_start"])
    assert same_bits(gpu.hop_sample_sqc(N, model, N_TRAJ - 100, SEED, *packet(c["p0"]), c["surface0"], code, gamma, trajectory_offset=100),
                     tuple(a[100:] for a in got))  # a slice with its offset
    dev = gpu.hop_sample_sqc(N, model, N_TRAJ, SEED, *packet(c["p0"]), c["surface0"], code, gamma, device_out=True)
    assert same_bits(tuple(t.cpu().numpy() for t in dev), got)  # device against host pointers


# ---- 2. parity per trajectory ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,window", BOTH)
def test_parity_per_trajectory(gpu, model_of, name, window):
    ref = reference(name, window)
    c, code, gamma, diag, D, want = ref["case"], ref["window"], ref["gamma"], ref["diag"], ref["D"], ref["end"]
    model, N = model_of(c), c["N"]
    per_status = np.bincount(want[4], minlength=3)
    assert diag["edge"].min() >= 1e-9, "a trajectory of the restatement decides its bound within rounding: change the case"
    assert ref["margin"] >= 1e-9, "an e of the restatement decides its window within rounding: change the case"
    got = gpu.hop_evolve_sqc(N, model, ref["start"], MASS, c["dt"], c["steps"], LEFT, RIGHT, gamma)  # one launch: the state never leaves the registers
    tol = [HN.tolerance(D[q], want[q]) for q in range(3)]
    err = [float(np.abs(got[q] - want[q]).max()) for q in range(3)]
    norm = np.abs(HM.norms(got[2]).sum(axis=1) - HM.norms(ref["start"][2]).sum(axis=1)).max()
    print(f"sqc parity {name} {window}: running / left / right {per_status}, windows none / k at the end {np.bincount(ref['window_end'] + 1, minlength=N + 1)}, "
          f"least distance to a bound {diag['edge'].min():.3g}, least window margin {ref['margin']:.3g}; D x {D[0]:.3g} p {D[1]:.3g} b {D[2]:.3g}; "
          f"err / tol x {err[0] / tol[0]:.3g} p {err[1] / tol[1]:.3g} b {err[2] / tol[2]:.3g}; norm drift {norm:.3g}")
    assert np.array_equal(got[4], want[4]) and got[4].dtype == np.int32
    assert got[3] is ref["start"][3]
    for q in range(3):
        assert err[q] <= tol[q], (name, "xpb"[q], err[q], tol[q])
    assert np.array_equal(device_windows(gpu, N, model, got, code, gamma), ref["window_end"])
    assert norm <= 1e-12


# ---- 3. observe -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", list(WINDOWS))
@pytest.mark.parametrize("name", ["dac10", "tsac0", "table3"])
def test_observe(gpu, model_of, name, window):
    ref = reference(name, window)
    c, code, gamma, state = ref["case"], ref["window"], ref["gamma"], ref["end"]
    model, N = model_of(c), c["N"]
    out = gpu.hop_observe_sqc(N, model, state, MASS, code, gamma)
    terms = HQ.observe_terms(ref["potential"], state, MASS, code, gamma)
    want = terms.sum(axis=0)
    assert out.shape == (4 * N + 9,)
    integers = slice(0, 3 * N + 6)
    assert np.array_equal(out[integers], want[integers])  # counts are exact
    counts, n_status, none = out[:3 * N].reshape(3, N), out[3 * N:3 * N + 3], out[3 * N + 3:3 * N + 6]
    assert np.array_equal(counts.sum(axis=1) + none, n_status) and np.array_equal(n_status, np.bincount(state[4], minlength=3)) and (n_status > 0).sum() >= 2
    assert none.sum() > 0 and (counts.sum(axis=0) > 0).sum() >= 2, "the case tests nothing"
    bound = N_TRAJ * EPS * np.abs(terms).sum(axis=0)[3 * N + 6:]
    err = np.abs(out - want)[3 * N + 6:]
    print(f"sqc observe {name} {window}: counts {counts.astype(int).tolist()} none {none.astype(int).tolist()}; err / tol of sum e, x, p, H {(err / bound).round(4).tolist()}")
    assert (err <= bound).all()
    assert np.array_equal(gpu.hop_observe_sqc(N, model, state, MASS, code, gamma), out)
    assert np.array_equal(gpu.hop_observe_sqc(N, model, on_device(gpu, *state), MASS, code, gamma), out)
    marked = state[:3] + (np.arange(N_TRAJ, dtype=np.int32) - 7,) + state[4:]  # the surface is not read
    assert np.array_equal(gpu.hop_observe_sqc(N, model, marked, MASS, code, gamma), out)
    odd = state[:4] + (np.where(np.arange(N_TRAJ) % 50 == 0, np.where(np.arange(N_TRAJ) % 100 == 0, 3, -1), state[4]).astype(np.int32),)
    skipped = gpu.hop_observe_sqc(N, model, odd, MASS, code, gamma)  # a status out of range adds nowhere
    keep = np.arange(N_TRAJ) % 50 != 0
    part = gpu.hop_observe_sqc(N, model, tuple(a[keep] for a in state), MASS, code, gamma)
    assert np.array_equal(skipped[integers], part[integers]) and skipped[3 * N:3 * N + 3].sum() == N_TRAJ - 6
    assert (np.abs(skipped - part)[3 * N + 6:] <= bound).all()


# ---- 4. bits --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,window", [("dac10", "triangle"), ("table3", "square")])
def test_bits(gpu, model_of, name, window):
    ref = reference(name, window)
    c, gamma, start = ref["case"], ref["gamma"], ref["start"]
    model = model_of(c)
    evolve = lambda state, steps: gpu.hop_evolve_sqc(c["N"], model, state, MASS, c["dt"], steps, LEFT, RIGHT, gamma)
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


# ---- 5. groups ------------------------------------------------------------------------------------------------------------------------------------
GROUPS = {"5x67": dict(N=2, model=HN.DAC, tabulated=False, window="triangle", p0=[8.0, 10.0, 16.0, 24.0, 30.0], dt=[2.0, 2.0, 1.0, 1.0, 0.5], steps=1500),
          "130x1": dict(N=3, model=HN.TSAC, tabulated=True, window="square", p0=list(np.linspace(8.0, 14.0, 130)), dt=list(np.where(np.arange(130) % 3 == 0, 4.0, 2.0)),
                        steps=800),
          "2x300": dict(N=2, model=HN.DAC, tabulated=False, window="square", p0=[10.0, 24.0], dt=[2.0, 1.0], steps=800)}


@pytest.mark.parametrize("shape", list(GROUPS))
def test_groups_are_the_plain_calls_on_slices(gpu, model_of, shape):
    c = GROUPS[shape]
    n_groups, n_per = (int(v) for v in shape.split("x"))
    model, N, steps, dt = model_of(c), c["N"], c["steps"], np.array(c["dt"])
    code = WINDOWS[c["window"]]
    gamma = HQ.GAMMA[code]
    p0 = np.array(c["p0"])
    packets = np.stack([np.full(n_groups, X0), p0, 1.0 / (2.0 * p0 / 20.0), p0 / 20.0], axis=1)
    start = gpu.hop_sample_groups_sqc(N, model, n_per, SEED, packets, 0, code, gamma)
    plain = gpu.hop_sample_groups(N, model, n_per, SEED, packets, 0)
    assert same_bits((start[0], start[1], start[3], start[4]), (plain[0], plain[1], plain[3], plain[4]))
    slices = HS.slices(n_groups, n_per)
    for g, sl in list(enumerate(slices))[:5]:                                             # differing packets: the plain sample per group
        assert same_bits(gpu.hop_sample_sqc(N, model, n_per, SEED, *packets[g], 0, code, gamma, trajectory_offset=g * n_per), tuple(a[sl] for a in start)), g
    equal = np.tile(packets[:1], (n_groups, 1))                                           # equal packets: the plain sample over the whole
    assert same_bits(gpu.hop_sample_groups_sqc(N, model, n_per, SEED, equal, 0, code, gamma), gpu.hop_sample_sqc(N, model, n_groups * n_per, SEED, *equal[0], 0, code, gamma))
    still = packets.copy()
    still[:, 2:] = 0.0                                                                    # the sigma == 0 select
    fixed = gpu.hop_sample_groups_sqc(N, model, n_per, SEED, still, 0, code, gamma)
    assert np.array_equal(fixed[0], np.full(n_groups * n_per, X0)) and np.array_equal(fixed[1], np.repeat(p0, n_per))
    assert same_bits((fixed[0], fixed[1]), gpu.hop_sample_groups(N, model, n_per, SEED, still, 0)[:2])
    grouped = lambda state, table, count: gpu.hop_evolve_groups_sqc(N, model, state, n_per, MASS, table, count, LEFT, RIGHT, gamma)
    whole = gpu.hop_evolve_sqc(N, model, start, MASS, 2.0, steps, LEFT, RIGHT, gamma)   # one dt for all: the plain call over the whole
    assert same_bits(grouped(start, np.full(n_groups, 2.0), steps), whole)
    mixed = grouped(start, dt, steps)                                                      # differing dt: one plain call per group
    assert same_bits(grouped(grouped(start, dt, 150), dt, steps - 150), mixed) and mixed[3] is start[3]
    rows = gpu.hop_observe_groups_sqc(N, model, mixed, n_per, MASS, code, gamma)
    assert rows.shape == (n_groups, 4 * N + 9) and np.array_equal(gpu.hop_observe_groups_sqc(N, model, mixed, n_per, MASS, code, gamma), rows)
    assert (rows[:, 3 * N:3 * N + 3].sum(axis=1) == n_per).all()
    assert np.array_equal(rows[:, :3 * N].reshape(n_groups, 3, N).sum(axis=2) + rows[:, 3 * N + 3:3 * N + 6], rows[:, 3 * N:3 * N + 3])
    for g, sl in enumerate(slices):
        alone = gpu.hop_evolve_sqc(N, model, tuple(a[sl] for a in start), MASS, dt[g], steps, LEFT, RIGHT, gamma)
        assert same_bits(alone, tuple(a[sl] for a in mixed)), g
        assert np.array_equal(gpu.hop_observe_sqc(N, model, alone, MASS, code, gamma), rows[g]), g
    dev = on_device(gpu, *start)                                                           # device pointers
    out = grouped(dev, dt, steps)
    gpu.synchronize()
    assert all(o is d for o, d in zip(out, dev)) and same_bits(tuple(t.cpu().numpy() for t in out), mixed)
    assert np.array_equal(gpu.hop_observe_groups_sqc(N, model, out, n_per, MASS, code, gamma), rows)
    done = mixed[4] != 0
    print(f"sqc groups {shape}: finished {done.sum()} of {len(done)}; in no window {int(rows[:, 3 * N + 3:3 * N + 6].sum())}")
    assert done.any() and (~done).any(), "the case tests nothing"


# ---- 6. against the mean-field kernel ---------------------------------------------------------------------------------------------------------------
def test_gamma_zero_is_the_mean_field_step(gpu):
    """gamma = 0 on an ensemble of gple_hop_sample: the force is the mean-field one minus 0 tr Fd.  The two kernels are compiled apart, so the
    check is the case's tolerance (D of the restatement's mean-field evolution), not bits"""
    c = CASES["dac10"]
    pot = HN.builtin(c["model"], 2)
    start = gpu.hop_sample(2, c["model"], N_TRAJ, SEED, *packet(c["p0"]), 0)
    sqc = gpu.hop_evolve_sqc(2, c["model"], start, MASS, c["dt"], c["steps"], LEFT, RIGHT, 0.0)
    mf = gpu.hop_evolve_mf(2, c["model"], start, MASS, c["dt"], c["steps"], LEFT, RIGHT)
    narrow, _ = HM.evolve(pot, start, MASS, c["dt"], c["steps"], LEFT, RIGHT)
    wide, _ = HM.evolve(pot, widen(start), MASS, c["dt"], c["steps"], LEFT, RIGHT)
    tol = [HN.tolerance(np.abs(narrow[q] - wide[q]).max(), narrow[q]) for q in range(3)]
    err = [float(np.abs(sqc[q] - mf[q]).max()) for q in range(3)]
    print(f"sqc at gamma = 0 against mean field: running / left / right {np.bincount(mf[4], minlength=3)}; err / tol x {err[0] / tol[0]:.3g} p {err[1] / tol[1]:.3g} "
          f"b {err[2] / tol[2]:.3g}")
    assert np.array_equal(sqc[4], mf[4]) and (np.bincount(mf[4], minlength=3) >= 5).sum() >= 2
    assert all(err[q] <= tol[q] for q in range(3))


# ---- 7. GPLE_ERR_BAD_ARG --------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments(gpu):
    ref = reference("dac16", "square")
    lib, ctx = gpu.lib, gpu.ctx
    x, p, b, surface, status = (a.copy() for a in ref["start"])
    n_groups, n_per = 1, N_TRAJ
    out, rows = np.full(17, -1.0), np.full((1, 17), -1.0)
    before = tuple(a.copy() for a in (x, p, b, surface, status, out, rows))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    arrays = dict(x=x.ctypes.data_as(dp), p=p.ctypes.data_as(dp), b=b.ctypes.data_as(dp), status=status.ctypes.data_as(ip))
    sampled = dict(arrays, surface=surface.ctypes.data_as(ip))
    nan, inf = float("nan"), float("inf")
    tables = []  # keeps the tables of the calls alive

    def table(values):
        tables.append(np.ascontiguousarray(values, dtype=np.float64))
        return tables[-1].ctypes.data_as(dp)

    def sample(**kw):
        a = dict(num_pes=2, model=1, n=N_TRAJ, offset=0, seed=SEED, x0=X0, p0=16.0, sx=0.625, sp=0.8, surface0=0, window=0, gamma=0.3, flags=0, **sampled)
        a.update(kw)
        return lib.gple_hop_sample_sqc(ctx, a["num_pes"], a["model"], a["n"], a["offset"], a["seed"], a["x0"], a["p0"], a["sx"], a["sp"], a["surface0"], a["window"],
                                       a["gamma"], a["flags"], a["x"], a["p"], a["b"], a["surface"], a["status"])

    def sample_groups(**kw):
        a = dict(num_pes=2, model=1, groups=n_groups, per=n_per, offset=0, seed=SEED, packets=table([X0, 16.0, 0.625, 0.8]), surface0=0, window=0, gamma=0.3, flags=0,
                 **sampled)
        a.update(kw)
        return lib.gple_hop_sample_groups_sqc(ctx, a["num_pes"], a["model"], a["groups"], a["per"], a["offset"], a["seed"], a["packets"], a["surface0"], a["window"],
                                              a["gamma"], a["flags"], a["x"], a["p"], a["b"], a["surface"], a["status"])

    def evolve(**kw):
        a = dict(num_pes=2, model=1, n=N_TRAJ, mass=MASS, dt=1.0, steps=3, left=LEFT, right=RIGHT, gamma=0.3, flags=0, **arrays)
        a.update(kw)
        return lib.gple_hop_evolve_sqc(ctx, a["num_pes"], a["model"], a["n"], a["mass"], a["dt"], a["steps"], a["left"], a["right"], a["gamma"], a["flags"], a["x"],
                                       a["p"], a["b"], a["status"])

    def evolve_groups(**kw):
        a = dict(num_pes=2, model=1, groups=n_groups, per=n_per, mass=MASS, dt=table([1.0]), steps=3, left=LEFT, right=RIGHT, gamma=0.3, flags=0, **arrays)
        a.update(kw)
        return lib.gple_hop_evolve_groups_sqc(ctx, a["num_pes"], a["model"], a["groups"], a["per"], a["mass"], a["dt"], a["steps"], a["left"], a["right"], a["gamma"],
                                              a["flags"], a["x"], a["p"], a["b"], a["status"])

    def observe(**kw):
        a = dict(num_pes=2, model=1, n=N_TRAJ, mass=MASS, window=0, gamma=0.3, flags=0, out=out.ctypes.data_as(dp), **arrays)
        a.update(kw)
        return lib.gple_hop_observe_sqc(ctx, a["num_pes"], a["model"], a["n"], a["mass"], a["window"], a["gamma"], a["flags"], a["x"], a["p"], a["b"], a["status"],
                                        a["out"])

    def observe_groups(**kw):
        a = dict(num_pes=2, model=1, groups=n_groups, per=n_per, mass=MASS, window=0, gamma=0.3, flags=0, out=rows.ctypes.data_as(dp), **arrays)
        a.update(kw)
        return lib.gple_hop_observe_groups_sqc(ctx, a["num_pes"], a["model"], a["groups"], a["per"], a["mass"], a["window"], a["gamma"], a["flags"], a["x"], a["p"],
                                               a["b"], a["status"], a["out"])

    t = tabulated(HN.DAC, 2)
    mine = gpu.pes_define(2, t.x_first, t.dx, t.V, t.dV)
    try:
        models = [dict(num_pes=1), dict(num_pes=4), dict(model=-1), dict(model=3), dict(model=7), dict(model=_capi.PES_USER + 15), dict(model=mine, num_pes=3)]
        nulls = [{k: None} for k in arrays]
        sizes = [dict(n=0), dict(n=(1 << 32) + 1)]
        group_sizes = [dict(groups=0), dict(per=0), dict(groups=_capi.HOP_MAX_GROUPS + 1, per=1), dict(groups=65536, per=1 << 60),
                       dict(groups=5, per=(1 << 64) // 5 + 1), dict(groups=4, per=(1 << 30) + 1)]
        stepping = [dict(mass=0.0), dict(mass=-1.0), dict(mass=nan), dict(mass=inf), dict(left=RIGHT), dict(left=7.0), dict(left=nan), dict(right=nan),
                    dict(right=inf), dict(steps=(1 << 40) + 1)]
        reverse = [dict(flags=_capi.HOP_REVERSE)]
        gammas = [dict(gamma=nan), dict(gamma=inf), dict(gamma=-0.1)]
        windows = gammas + [dict(window=-1), dict(window=2), dict(window=0, gamma=0.0), dict(window=0, gamma=0.5), dict(window=0, gamma=0.7), dict(window=1, gamma=-1e-300)]
        sampling = [dict(surface0=-1), dict(surface0=2), dict(surface=None)]
        for kw in models + nulls + sizes + sampling + windows + reverse + [dict(offset=(1 << 32) - N_TRAJ + 1), dict(sx=0.0), dict(sp=-1.0), dict(sx=nan), dict(sp=inf)]:
            assert sample(**kw) == BAD_ARG, kw
        for kw in models + nulls + group_sizes + sampling + windows + reverse + [dict(packets=None)] + [dict(packets=table(v)) for v in
                                                                                                    ([nan, 1, 1, 1], [0, inf, 1, 1], [0, 1, -1, 1], [0, 1, 1, nan])]:
            assert sample_groups(**kw) == BAD_ARG, kw
        for kw in models + nulls + sizes + stepping + gammas + reverse + [dict(dt=0.0), dict(dt=-1.0), dict(dt=nan), dict(dt=inf)]:
            assert evolve(**kw) == BAD_ARG, kw
        for kw in models + nulls + group_sizes + stepping + gammas + reverse + [dict(dt=None)] + [dict(dt=table([v])) for v in (0.0, -1.0, nan, inf)]:
            assert evolve_groups(**kw) == BAD_ARG, kw
        assert evolve_groups(groups=2, per=100, dt=table([1.0, nan])) == BAD_ARG and evolve_groups(groups=2, per=100, dt=table([-1.0, 1.0])) == BAD_ARG
        for kw in models + nulls + sizes + windows + reverse + [dict(mass=0.0), dict(mass=nan), dict(mass=inf), dict(out=None)]:
            assert observe(**kw) == BAD_ARG, kw
        for kw in models + nulls + group_sizes + windows + reverse + [dict(mass=0.0), dict(mass=nan), dict(mass=inf), dict(out=None)]:
            assert observe_groups(**kw) == BAD_ARG, kw
        assert same_bits((x, p, b, surface, status, out, rows), before)  # a refused call writes nothing
        # what is not refused: the user model, no step at all, gamma = 0 and a large gamma where no square window is named
        assert evolve(steps=0) == 0 and evolve_groups(steps=0) == 0 and same_bits((x, p, b, surface, status), before[:5])
        assert observe(model=mine) == 0 and observe_groups(model=mine) == 0 and np.array_equal(out, rows[0]) and out[6:9].sum() == N_TRAJ
        assert observe(window=1, gamma=0.0) == 0 and observe(window=1, gamma=3.0) == 0
        assert evolve(model=mine, gamma=0.0) == 0 and not np.array_equal(x, before[0])
        assert evolve_groups(gamma=3.0) == 0
        assert sample(window=1, gamma=0.0) == 0 and sample_groups(model=mine, window=1, gamma=2.0, packets=table([X0, 16.0, 0.0, 0.0])) == 0 and (x == X0).all()
    finally:
        gpu.pes_undefine(mine)


# ---- 8. the driver --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", list(WINDOWS))
def test_driver_against_the_same_loop_on_the_restatement(gpu, tmp_path, window):
    kw = dict(model=hopping.DAC, num_pes=2, ln_energy=-2.0, n_traj=512, seed=SEED, dt=2.0, x0=X0, xmin=LEFT, xmax=RIGHT, method="sqc", window=window)
    res = hopping.run(gpu, out_dir=str(tmp_path), **kw)
    narrow = hopping.run(HQ.NumpySqcApi(), **kw)
    wide = hopping.run(HQ.NumpySqcApi(dtype=np.longdouble), **kw)
    assert res["stop"] is not None and res["stop"] == narrow["stop"] == wide["stop"] and len(res["records"]) == len(narrow["records"]) == len(wide["records"]) > 10
    assert hasattr(res["state"][0], "is_cuda") and res["state"][0].is_cuda  # the ensemble stayed on the device
    worst = {}
    for key in ("x", "p", "E", "e"):
        got, f64, ld = (np.array([r[key] for r in run["records"]]) for run in (res, narrow, wide))
        tol = HN.tolerance(np.abs(f64 - ld).max(), f64)
        worst[key] = np.abs(got - f64).max() / tol
    print("sqc driver %s: %d outputs; err / tol %s" % (window, len(res["records"]), ", ".join(f"{k} {v:.3g}" for k, v in worst.items())))
    for a, b in zip(res["records"], narrow["records"]):  # the integers are exact, as long as the three runs agree on every window
        assert a["t"] == b["t"] and all(np.array_equal(a[key], b[key]) for key in ("counts", "n_status", "none"))
    assert all(v <= 1.0 for v in worst.values()), worst
    assert res["scattering_line"] == narrow["scattering_line"]
    line = [float(v) for v in res["scattering_line"].split()]
    assert len(line) == 7 and abs(sum(line[1:5]) - 1.0) < 1e-5 and line[5] == 0.0 and 0.0 < line[6] < 1.0
    t = [float(l) for l in open(tmp_path / "t.txt")]
    av = [[float(v) for v in l.split()] for l in open(tmp_path / "averages.txt")]
    assert len(t) == len(av) == len(res["records"])
    for rec, tt, row in zip(res["records"], t, av):
        assert np.allclose([tt] + row, [rec["t"], rec["t"], rec["E"], rec["x"], rec["p"], *rec["windowed"], *rec["actions"], rec["unassigned"]], rtol=1e-5, atol=1e-300)
