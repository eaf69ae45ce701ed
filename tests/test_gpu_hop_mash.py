"""GPU: MASH trajectories (gple_hop_sample_mash / _evolve_mash and their _groups forms, csrc/gple_hop.hip; DESIGN.md §17, "MASH trajectories")
against the numpy restatement tests/hop_mash_numpy.py, trajectory by trajectory, and against themselves bit for bit.

Every ensemble is that of tests/hop_mash_cases.py: 293 trajectories (a tail that is no multiple of 64 or 256), seed 0, x0 = -4, sigma_p = p0 / 20,
bounds +-6, mass 2000, on the two-level cases of tests/test_gpu_hop.py.  Decisions (surface, status, the numbers of hops taken and of frustrated
hops) must be EQUAL; x, p and b lie within 64 D_q + 1e-13 max(1, max|q|), D_q being the largest distance between the float64 and the long double
restatement for that quantity and case, computed here.  A trajectory is set aside only where the float64 restatement's own margin is too small:
its least | |c_1|^2 - |c_0|^2 | below 1e-10, or an attempted hop with |r| < 1e-9 p^2; at most 2 of 293 per case may be, which is asserted
(tests/test_hop_mash_host.py shows without a GPU that seed 0 sets none aside).  The figures measured on the MI355X are in DESIGN.md §17."""
import ctypes as C

import numpy as np
import pytest

from gaussian_process_liouville_equation_amd import _capi, hopping
from tests import hop_mash_cases as HC
from tests import hop_mash_numpy as HA
from tests import hop_numpy as HN
from tests import hop_scan_numpy as HS
from tests.hop_mash_cases import CASES, LEFT, MASS, N_TRAJ, RIGHT, SEED, X0, packet, reference

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
BAD_ARG = 1


@pytest.fixture
def model_of(gpu):
    """model_of(case) -> the id on the session's context (a table is defined, and undefined when the test ends)"""
    ids = []

    def make(c):
        if not c["tabulated"]:
            return c["model"]
        t = HC.tabulated(c["model"])
        ids.append(gpu.pes_define(2, t.x_first, t.dx, t.V, t.dV))
        return ids[-1]

    yield make
    for model in ids:
        gpu.pes_undefine(model)


def same_bits(a, b):
    return all(np.array_equal(u, v) and u.dtype == v.dtype for u, v in zip(a, b))


def on_device(gpu, *arrays):
    import torch

    where = torch.device("cuda", gpu.device)
    out = tuple(torch.from_numpy(np.ascontiguousarray(a).copy()).to(where) for a in arrays)
    torch.cuda.synchronize(where)
    return out


# ---- 1. the sample ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_sample(gpu, model_of, name):
    ref = reference(name)
    c, want = ref["case"], ref["start"]
    model = model_of(c)
    got = gpu.hop_sample_mash(2, model, N_TRAJ, SEED, *packet(c["p0"]), c["surface0"])
    plain = gpu.hop_sample(2, model, N_TRAJ, SEED, *packet(c["p0"]), c["surface0"])
    assert same_bits((got[0], got[1], got[3], got[4]), (plain[0], plain[1], plain[3], plain[4]))  # x and p have the bits of gple_hop_sample
    assert (got[3] == c["surface0"]).all() and (got[4] == 0).all() and got[3].dtype == got[4].dtype == np.int32
    tol, err = HN.tolerance(ref["D_sample"], want[2]), float(np.abs(got[2] - want[2]).max())
    print(f"mash sample {name}: D b {ref['D_sample']:.3g}; err / tol b {err / tol:.3g}")
    assert err <= tol
    assert np.abs(HA.norms(got[2]).sum(axis=1) - 1.0).max() <= 8 * EPS
    _, _, Cm, _ = HN.states(got[0], ref["potential"])  # the adiabatic states at the device's own x
    assert np.array_equal(HA.side(HA.adiabatic(Cm, got[2])), np.full(N_TRAJ, c["surface0"]))
    assert same_bits(gpu.hop_sample_mash(2, model, N_TRAJ - 100, SEED, *packet(c["p0"]), c["surface0"], trajectory_offset=100),
                     tuple(a[100:] for a in got))  # a slice with its offset
    dev = gpu.hop_sample_mash(2, model, N_TRAJ, SEED, *packet(c["p0"]), c["surface0"], device_out=True)
    assert same_bits(tuple(t.cpu().numpy() for t in dev), got)  # device against host pointers
    assert same_bits(gpu.hop_sample_mash(2, model, N_TRAJ, SEED, *packet(c["p0"]), c["surface0"]), got)  # a repeat
    assert not np.array_equal(gpu.hop_sample_mash(2, model, N_TRAJ, SEED + 1, *packet(c["p0"]), c["surface0"])[2], got[2])


# ---- 2. parity per trajectory ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_parity_per_trajectory(gpu, model_of, name):
    ref = reference(name)
    c, diag, D, want, keep = ref["case"], ref["diag"], ref["D"], ref["end"], ~ref["aside"]
    model = model_of(c)
    assert diag["hops"].sum() >= 10, "the case tests nothing"
    if name == "dac10":
        assert diag["frustrated"].sum() >= 10, "the case tests nothing"
    assert ref["aside"].sum() <= 2
    got = gpu.hop_evolve_mash(2, model, ref["start"], MASS, c["dt"], c["steps"], LEFT, RIGHT)  # one launch: the state never leaves the registers
    # the counts of taken and of frustrated hops, from the grouped call over one group; by the way the same bits
    counted, hops = gpu.hop_evolve_groups_mash(2, model, ref["start"], N_TRAJ, MASS, np.array([c["dt"]]), c["steps"], LEFT, RIGHT,
                                               hops=np.zeros((N_TRAJ, 2), dtype=np.int32))
    assert same_bits(counted, got)
    tol = [HN.tolerance(D[q], want[q]) for q in range(3)]
    err = [float(np.abs(got[q] - want[q])[keep].max()) for q in range(3)]
    print(f"mash parity {name}: hops {diag['hops'].sum()} frustrated {diag['frustrated'].sum()} running / left / right {np.bincount(want[4], minlength=3)} "
          f"least side margin {diag['margin'].min():.3g} least |r| / p^2 {diag['ratio'].min():.3g} set aside {ref['aside'].sum()}; "
          f"D x {D[0]:.3g} p {D[1]:.3g} b {D[2]:.3g}; err / tol x {err[0] / tol[0]:.3g} p {err[1] / tol[1]:.3g} b {err[2] / tol[2]:.3g}; "
          f"least distance to a bound {diag['edge'].min():.3g}")
    assert np.array_equal(got[3][keep], want[3][keep]) and np.array_equal(got[4][keep], want[4][keep]) and got[3].dtype == got[4].dtype == np.int32
    assert np.array_equal(hops[keep, 0], diag["hops"][keep]) and np.array_equal(hops[keep, 1], diag["frustrated"][keep])
    for q in range(3):
        assert err[q] <= tol[q], (name, "xpb"[q], err[q], tol[q])
    assert np.abs(HA.norms(got[2]).sum(axis=1) - 1.0).max() <= 1e-12


# ---- 3. bits --------------------------------------------------------------------------------------------------------------------------------------
def test_bits(gpu, model_of):
    ref = reference("dac10")
    c, start = ref["case"], ref["start"]
    model = model_of(c)
    evolve = lambda state, steps: gpu.hop_evolve_mash(2, model, state, MASS, c["dt"], steps, LEFT, RIGHT)
    steps = 400
    whole = evolve(start, steps)
    state = start
    for _ in range(steps):  # one launch per step: the cuts fall between a reflection and the crossing back too
        state = evolve(state, 1)
    assert same_bits(state, whole)
    assert same_bits(evolve(start, steps), whole)                                        # a repeat
    assert same_bits(evolve(tuple(a[100:] for a in start), steps), tuple(a[100:] for a in whole))  # a slice against the whole
    dev = on_device(gpu, *start)                                                         # device against host pointers
    out = evolve(dev, steps)
    gpu.synchronize()
    assert all(o is d for o, d in zip(out, dev))
    assert same_bits(tuple(t.cpu().numpy() for t in out), whole)
    end = evolve(whole, c["steps"] - steps)                                              # a finished trajectory is frozen
    done = end[4] != 0
    assert done.sum() >= 10 and (~done).sum() >= 10
    later = evolve(end, 200)
    assert same_bits(tuple(a[done] for a in later), tuple(a[done] for a in end)) and not np.array_equal(later[0][~done], end[0][~done])
    assert same_bits(end, evolve(start, c["steps"]))


# ---- 4. groups ------------------------------------------------------------------------------------------------------------------------------------
def test_groups_are_the_plain_calls_on_slices(gpu, model_of):
    c = dict(model=HN.DAC, tabulated=False)
    n_groups, n_per, steps = 5, 67, 1000
    model = model_of(c)
    p0, dt = np.array([8.0, 10.0, 10.0, 16.0, 24.0]), np.array([2.0, 2.0, 1.0, 1.0, 0.5])
    packets = np.stack([np.full(n_groups, X0), p0, 1.0 / (2.0 * p0 / 20.0), p0 / 20.0], axis=1)
    n = n_groups * n_per
    start = gpu.hop_sample_groups_mash(2, model, n_per, SEED, packets, 0)
    plain = gpu.hop_sample_groups(2, model, n_per, SEED, packets, 0)
    assert same_bits((start[0], start[1], start[3], start[4]), (plain[0], plain[1], plain[3], plain[4]))
    slices = HS.slices(n_groups, n_per)
    for g, sl in enumerate(slices):                                                       # the grouped sample is the plain one, slice by slice
        assert same_bits(gpu.hop_sample_mash(2, model, n_per, SEED, *packets[g], 0, trajectory_offset=g * n_per), tuple(a[sl] for a in start)), g
    equal = np.tile(packets[:1], (n_groups, 1))                                           # equal packets: the plain sample over the whole
    assert same_bits(gpu.hop_sample_groups_mash(2, model, n_per, SEED, equal, 0), gpu.hop_sample_mash(2, model, n, SEED, *equal[0], 0))
    still = packets.copy()
    still[:, 2:] = 0.0                                                                    # the sigma == 0 select
    fixed = gpu.hop_sample_groups_mash(2, model, n_per, SEED, still, 0)
    assert np.array_equal(fixed[0], np.full(n, X0)) and np.array_equal(fixed[1], np.repeat(p0, n_per))
    dev = gpu.hop_sample_groups_mash(2, model, n_per, SEED, packets, 0, device_out=True)
    assert same_bits(tuple(t.cpu().numpy() for t in dev), start)
    zeros = np.zeros((n, 2), dtype=np.int32)
    grouped = lambda state, table, count, **kw: gpu.hop_evolve_groups_mash(2, model, state, n_per, MASS, table, count, LEFT, RIGHT, **kw)
    whole = gpu.hop_evolve_mash(2, model, start, MASS, 2.0, steps, LEFT, RIGHT)           # one dt for all: the plain call over the whole
    assert same_bits(grouped(start, np.full(n_groups, 2.0), steps), whole)
    mixed, hops = grouped(start, dt, steps, hops=zeros)                                   # differing dt: one plain call per group
    assert same_bits(grouped(start, dt, steps), mixed)                                    # hops = null: the same state
    for g, sl in enumerate(slices):
        assert same_bits(gpu.hop_evolve_mash(2, model, tuple(a[sl] for a in start), MASS, dt[g], steps, LEFT, RIGHT), tuple(a[sl] for a in mixed)), g
    first, h1 = grouped(start, dt, 150, hops=zeros)                                       # hops accumulate over two calls
    second, h2 = grouped(first, dt, steps - 150, hops=h1)
    assert same_bits(second, mixed) and np.array_equal(h2, hops) and h2.dtype == np.int32 and not zeros.any()
    assert hops[:, 0].sum() >= 10 and hops[:, 1].sum() >= 10 and (h1 != hops).any()
    _, more = grouped(start, dt, steps, hops=np.full((n, 2), 3, dtype=np.int32))          # added to what is there
    assert np.array_equal(more, hops + 3)
    pot = HN.builtin(HN.DAC, 2)
    _, want, diag = HA.evolve_groups(pot, start, n_per, MASS, dt, steps, LEFT, RIGHT)    # the counters of the restatement on the device's own sample
    keep = ~HA.set_aside(diag)
    assert (~keep).sum() <= 2 and np.array_equal(hops[keep], want[keep])
    dev = on_device(gpu, *start)                                                          # device pointers, the counters on the device too
    counters = on_device(gpu, zeros)[0]
    out, counted = grouped(dev, dt, steps, hops=counters)
    gpu.synchronize()
    assert all(o is d for o, d in zip(out, dev)) and counted is counters
    assert same_bits(tuple(t.cpu().numpy() for t in out), mixed) and np.array_equal(counters.cpu().numpy(), hops)
    rows = gpu.hop_observe_groups(2, model, mixed, n_per, MASS)                           # the existing grouped sums serve the ensemble
    for g, sl in enumerate(slices):
        assert np.array_equal(gpu.hop_observe(2, model, tuple(a[sl] for a in mixed), MASS), rows[g]), g
    done = mixed[4] != 0
    print(f"mash groups 5x67: finished {done.sum()} of {n}; hops {hops[:, 0].sum()} frustrated {hops[:, 1].sum()}")
    assert done.any() and (~done).any(), "the case tests nothing"


# ---- 5. observe -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dac10", "ecr", "table2"])
def test_observe(gpu, model_of, name):
    ref = reference(name)
    c, state = ref["case"], ref["end"]
    model = model_of(c)
    out = gpu.hop_observe(2, model, state, MASS)
    terms = HN.observe_terms(ref["potential"], state, MASS)
    assert out.shape == (11,)
    assert np.array_equal(out[:6], terms[:, :6].sum(axis=0)) and out[:6].sum() == N_TRAJ  # counts of the active surface are exact
    assert (out[:6].reshape(3, 2).sum(axis=0) > 0).all()  # both surfaces are active somewhere
    bound = N_TRAJ * EPS * np.abs(terms[:, 6:]).sum(axis=0)
    err = np.abs(out[6:] - terms[:, 6:].sum(axis=0))
    print(f"mash observe {name}: counts {out[:6].astype(int).tolist()}; err / tol {np.max(err / bound):.3g}")
    assert (err <= bound).all()
    assert np.array_equal(gpu.hop_observe(2, model, on_device(gpu, *state), MASS), out)


# ---- 6. GPLE_ERR_BAD_ARG --------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments(gpu):
    ref = reference("dac16")
    lib, ctx = gpu.lib, gpu.ctx
    x, p, b, surface, status = (a.copy() for a in ref["start"])
    b3 = np.zeros((N_TRAJ, 3), dtype=np.complex128)
    hops = np.full((N_TRAJ, 2), 5, dtype=np.int32)
    before = tuple(a.copy() for a in (x, p, b, surface, status, hops, b3))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    arrays = dict(x=x.ctypes.data_as(dp), p=p.ctypes.data_as(dp), b=b.ctypes.data_as(dp), surface=surface.ctypes.data_as(ip), status=status.ctypes.data_as(ip))
    nan, inf = float("nan"), float("inf")
    tables = []  # keeps the tables of the calls alive

    def table(values):
        tables.append(np.ascontiguousarray(values, dtype=np.float64))
        return tables[-1].ctypes.data_as(dp)

    def sample(**kw):
        a = dict(num_pes=2, model=1, n=N_TRAJ, offset=0, seed=SEED, x0=X0, p0=16.0, sx=0.625, sp=0.8, surface0=0, flags=0, **arrays)
        a.update(kw)
        return lib.gple_hop_sample_mash(ctx, a["num_pes"], a["model"], a["n"], a["offset"], a["seed"], a["x0"], a["p0"], a["sx"], a["sp"], a["surface0"], a["flags"],
                                        a["x"], a["p"], a["b"], a["surface"], a["status"])

    def sample_groups(**kw):
        a = dict(num_pes=2, model=1, groups=1, per=N_TRAJ, offset=0, seed=SEED, packets=table([X0, 16.0, 0.625, 0.8]), surface0=0, flags=0, **arrays)
        a.update(kw)
        return lib.gple_hop_sample_groups_mash(ctx, a["num_pes"], a["model"], a["groups"], a["per"], a["offset"], a["seed"], a["packets"], a["surface0"], a["flags"],
                                               a["x"], a["p"], a["b"], a["surface"], a["status"])

    def evolve(**kw):
        a = dict(num_pes=2, model=1, n=N_TRAJ, mass=MASS, dt=1.0, steps=3, left=LEFT, right=RIGHT, flags=0, **arrays)
        a.update(kw)
        return lib.gple_hop_evolve_mash(ctx, a["num_pes"], a["model"], a["n"], a["mass"], a["dt"], a["steps"], a["left"], a["right"], a["flags"], a["x"], a["p"],
                                        a["b"], a["surface"], a["status"])

    def evolve_groups(**kw):
        a = dict(num_pes=2, model=1, groups=1, per=N_TRAJ, mass=MASS, dt=table([1.0]), steps=3, left=LEFT, right=RIGHT, flags=0, hops=hops.ctypes.data_as(ip), **arrays)
        a.update(kw)
        return lib.gple_hop_evolve_groups_mash(ctx, a["num_pes"], a["model"], a["groups"], a["per"], a["mass"], a["dt"], a["steps"], a["left"], a["right"], a["flags"],
                                               a["x"], a["p"], a["b"], a["surface"], a["status"], a["hops"])

    t = HC.tabulated(HN.DAC)
    mine = gpu.pes_define(2, t.x_first, t.dx, t.V, t.dV)
    try:
        levels = [dict(num_pes=3, model=3, b=b3.ctypes.data_as(dp)), dict(num_pes=3), dict(num_pes=1), dict(num_pes=4)]  # three levels: refused, TSAC included
        models = levels + [dict(model=-1), dict(model=3), dict(model=7), dict(model=_capi.PES_USER + 15)]
        nulls = [{k: None} for k in arrays]
        sizes = [dict(n=0), dict(n=(1 << 32) + 1)]
        group_sizes = [dict(groups=0), dict(per=0), dict(groups=_capi.HOP_MAX_GROUPS + 1, per=1), dict(groups=65536, per=1 << 60), dict(groups=4, per=(1 << 30) + 1)]
        stepping = [dict(mass=0.0), dict(mass=-1.0), dict(mass=nan), dict(mass=inf), dict(left=RIGHT), dict(left=7.0), dict(left=nan), dict(right=nan),
                    dict(right=inf), dict(steps=(1 << 40) + 1)]
        reverse = [dict(flags=_capi.HOP_REVERSE)]
        sampling = [dict(surface0=-1), dict(surface0=2)]
        for kw in models + nulls + sizes + sampling + reverse + [dict(offset=(1 << 32) - N_TRAJ + 1), dict(sx=0.0), dict(sp=-1.0), dict(sx=nan), dict(sp=inf)]:
            assert sample(**kw) == BAD_ARG, kw
        for kw in models + nulls + group_sizes + sampling + reverse + [dict(packets=None)] + [dict(packets=table(v)) for v in
                                                                                             ([nan, 1, 1, 1], [0, inf, 1, 1], [0, 1, -1, 1], [0, 1, 1, nan])]:
            assert sample_groups(**kw) == BAD_ARG, kw
        for kw in models + nulls + sizes + stepping + reverse + [dict(dt=0.0), dict(dt=-1.0), dict(dt=nan), dict(dt=inf)]:
            assert evolve(**kw) == BAD_ARG, kw
        for kw in models + nulls + group_sizes + stepping + reverse + [dict(dt=None)] + [dict(dt=table([v])) for v in (0.0, -1.0, nan, inf)]:
            assert evolve_groups(**kw) == BAD_ARG, kw
        assert evolve_groups(groups=2, per=100, dt=table([1.0, nan])) == BAD_ARG and evolve_groups(groups=2, per=100, dt=table([-1.0, 1.0])) == BAD_ARG
        assert same_bits((x, p, b, surface, status, hops, b3), before)  # a refused call writes nothing
        # what is not refused: no step at all, the user model, hops = null
        assert evolve(steps=0) == 0 and evolve_groups(steps=0) == 0 and same_bits((x, p, b, surface, status, hops), before[:6])
        assert evolve(model=mine) == 0 and not np.array_equal(x, before[0])
        assert evolve_groups(hops=None) == 0 and np.array_equal(hops, before[5])
        assert sample_groups(model=mine, packets=table([X0, 16.0, 0.0, 0.0])) == 0 and (x == X0).all() and (p == 16.0).all()
        assert sample() == 0 and (status == 0).all() and (surface == 0).all() and len(np.unique(x)) == N_TRAJ
    finally:
        gpu.pes_undefine(mine)
    with pytest.raises(ValueError):
        hopping.run(gpu, method="mash", num_pes=3, model=hopping.TSAC)


# ---- 7. the driver --------------------------------------------------------------------------------------------------------------------------------
def test_driver_against_the_same_loop_on_the_restatement(gpu, tmp_path):
    kw = dict(model=hopping.DAC, num_pes=2, ln_energy=-2.0, n_traj=512, seed=SEED, dt=2.0, x0=X0, xmin=LEFT, xmax=RIGHT, method="mash")
    res = hopping.run(gpu, out_dir=str(tmp_path), **kw)
    narrow = hopping.run(HA.NumpyMashApi(), **kw)
    wide = hopping.run(HA.NumpyMashApi(dtype=np.longdouble), **kw)
    assert res["stop"] is not None and res["stop"] == narrow["stop"] == wide["stop"] and len(res["records"]) == len(narrow["records"]) == len(wide["records"]) > 10
    assert hasattr(res["state"][0], "is_cuda") and res["state"][0].is_cuda  # the ensemble stayed on the device
    worst = {}
    for key in ("x", "p", "E", "populations"):
        got, f64, ld = (np.array([r[key] for r in run["records"]]) for run in (res, narrow, wide))
        tol = HN.tolerance(np.abs(f64 - ld).max(), f64)
        worst[key] = np.abs(got - f64).max() / tol
    print("mash driver: %d outputs; err / tol %s" % (len(res["records"]), ", ".join(f"{k} {v:.3g}" for k, v in worst.items())))
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


def test_scan_against_the_same_loop_on_the_restatement(gpu, tmp_path):
    """hopping.scan(method="mash") with the ensemble and the counters of hops on the device, against the stand-in: the integers are equal as long
    as no decision of the restatement is within rounding, which its margins show"""
    kw = dict(model=hopping.DAC, num_pes=2, momenta=[10.0, 16.0, 30.0], n_per_group=67, seed=SEED, dt=[2.0, 1.0, 1.0], x0=X0, xmin=LEFT, xmax=RIGHT, fixed=False,
              chunk_steps=256, max_steps=1024, method="mash")
    res = hopping.scan(gpu, out_dir=str(tmp_path), **kw)
    want = hopping.scan(HA.NumpyMashApi(), **kw)
    assert res["stop"] == want["stop"] and res["steps"] == want["steps"] == 1024 and (want["rows"][:, 2:6].sum(axis=1) > 0).all()  # every group has finished ones
    assert hasattr(res["state"][0], "is_cuda") and res["state"][0].is_cuda and res["hop_counts"].is_cuda  # the ensemble and its counters stayed on the device
    pot = HN.builtin(HN.DAC, 2)
    _, _, diag = HA.evolve_groups(pot, HA.sample_groups(pot, 2, 67, SEED, [[s["x0"], s["p0"], s["sigma_x"], s["sigma_p"]] for s in want["setups"]], 0), 67, MASS,
                                  want["dt"], want["steps"], LEFT, RIGHT)
    assert not HA.set_aside(diag).any(), "a trajectory of the restatement decides within rounding: change the seed"
    assert np.array_equal(res["rows"][:, :6], want["rows"][:, :6]) and np.array_equal(res["scattered"], want["scattered"])
    assert np.array_equal(res["hops"], want["hops"]) and np.array_equal(res["frustrated"], want["frustrated"]) and res["hops"].sum() > 0
    assert np.array_equal(res["hop_counts"].cpu().numpy(), want["hop_counts"])
    print(f"mash scan: {res['steps']} steps; hops per trajectory {res['hops'].round(3).tolist()} frustrated {res['frustrated'].round(3).tolist()}; "
          f"largest difference of a real sum {np.abs(res['rows'][:, 6:] - want['rows'][:, 6:]).max():.3g}")
    lines = [[float(v) for v in l.split()] for l in open(tmp_path / "scan.txt")]
    assert len(lines) == 3 and all(len(line) == 14 for line in lines)
    assert [l.split()[:11] for l in res["lines"]] == [l.split()[:11] for l in want["lines"]]  # the head, the fractions and their standard errors: the same text
