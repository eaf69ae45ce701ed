"""GPU: grouped surface hopping ensembles (gple_hop_sample_groups / _evolve_groups / _observe_groups, csrc/gple_hop.hip; DESIGN.md §17, "A curve
in one launch") against the plain calls on slices, bit for bit, against the numpy restatement tests/hop_scan_numpy.py, and the driver
hopping.scan against itself on the numpy stand-in api.

Shapes: 5 groups x 67 trajectories (group edges inside waves and inside a 256-thread workgroup of a flat launch), 130 x 1 (more groups than lanes
of a wave) and 2 x 300 (a group spanning workgroups).  x0 = -4, sigma_p = p0 / 20, bounds +-6, mass 2000, seed 0, as tests/test_gpu_hop.py.  The
direct comparison follows that file's rule: decisions (surface, status, both hop counters) EQUAL, x, p, b within 64 D_q + 1e-13 max(1, max|q|)
with D_q the float64-to-long-double distance of the restatement, computed here; a trajectory is set aside only where the float64 restatement's
own margin |xi - (g_1 + ... + g_k)| is below 1e-10, at most 1 % of the case may be, and with these inputs none is (least margin 1.3e-6, checked
on the host first)."""
import ctypes as C
import functools

import numpy as np
import pytest

from gaussian_process_liouville_equation_amd import _capi, hopping, pes
from tests import hop_numpy as HN
from tests import hop_scan_numpy as HS

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
X0, MASS, LEFT, RIGHT, SEED = -4.0, 2000.0, -6.0, 6.0, 0
BAD_ARG = 1
SHAPES = {"5x67": (5, 67), "130x1": (130, 1), "2x300": (2, 300)}
DAC_P0 = {"5x67": [8.0, 10.0, 16.0, 24.0, 30.0], "130x1": list(np.linspace(8.0, 30.0, 130)), "2x300": [10.0, 24.0]}
LAST = (1 << 32)  # the end of the index space


def dac_dt(p0):
    return 2.0 if p0 < 13.0 else 1.0 if p0 < 27.0 else 0.5


@functools.lru_cache(maxsize=None)
def case(name, shape):
    """name: dac, dac-reverse, tsac (three levels from the middle surface), table (DAC tabulated at dx = 1 / 16), fixed (sigma_x = sigma_p = 0)"""
    n_groups, n_per = SHAPES[shape]
    c = dict(name=name, N=2, model=HN.DAC, tabulated=name == "table", surface0=0, reverse=name == "dac-reverse", steps=900, offset=0, n_groups=n_groups,
             n_per=n_per, n=n_groups * n_per)
    p0 = np.array(DAC_P0[shape])
    c["dt"] = np.array([dac_dt(v) for v in p0])
    if name == "tsac":
        p0 = np.linspace(8.0, 14.0, n_groups)
        c.update(N=3, model=HN.TSAC, surface0=1, steps=250, dt=np.where(p0 < 11.0, 4.0, 2.0), offset=LAST - c["n"])  # the last admissible offset
    if name == "dac-reverse":
        c["offset"] = 1000
    sigma = 0.0 if name == "fixed" else 1.0
    c["packets"] = np.stack([np.full(n_groups, X0), p0, sigma / (2.0 * p0 / 20.0), sigma * p0 / 20.0], axis=1)
    c["potential"] = HN.table(tabulated(c["model"], c["N"])) if c["tabulated"] else HN.builtin(c["model"], c["N"])
    c["start"] = HS.sample_groups(c["potential"], c["N"], n_per, SEED, c["packets"], c["surface0"], c["offset"])
    return c


CASES = [("dac", "5x67"), ("dac-reverse", "5x67"), ("tsac", "130x1"), ("table", "2x300"), ("fixed", "5x67"), ("dac", "130x1"), ("dac", "2x300")]


@functools.lru_cache(maxsize=None)
def tabulated(model, N):
    """pes.tabulate of a built-in model on [-8, 8] at dx = 1 / 16"""
    return HN.FunctionTable(*pes.tabulate(HN.scalar_function(HN.builtin(model, N)), -8.0, 1.0 / 16.0, 257))


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


def on_device(gpu, *arrays):
    import torch

    where = torch.device("cuda", gpu.device)
    out = tuple(torch.from_numpy(np.ascontiguousarray(a).copy()).to(where) for a in arrays)
    torch.cuda.synchronize(where)
    return out


def widen(state):
    x, p, b, surface, status = state
    return x.astype(np.longdouble), p.astype(np.longdouble), b.astype(np.clongdouble), surface, status


# ---- 1. sample ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,shape", CASES)
def test_sample_bits(gpu, model_of, name, shape):
    c = case(name, shape)
    model, N, n_per = model_of(c), c["N"], c["n_per"]
    got = gpu.hop_sample_groups(N, model, n_per, SEED, c["packets"], c["surface0"], trajectory_offset=c["offset"])
    x, p, b, surface, status = got
    assert (surface == c["surface0"]).all() and (status == 0).all() and (b.imag == 0).all()
    assert same_bits(gpu.hop_sample_groups(N, model, n_per, SEED, c["packets"], c["surface0"], trajectory_offset=c["offset"]), got)  # a repeat
    dev = gpu.hop_sample_groups(N, model, n_per, SEED, c["packets"], c["surface0"], trajectory_offset=c["offset"], device_out=True)
    assert same_bits(tuple(t.cpu().numpy() for t in dev), got)  # device pointers
    if name != "fixed":
        for g, sl in enumerate(HS.slices(c["n_groups"], n_per)):  # with positive sigmas: gple_hop_sample on the slice
            plain = gpu.hop_sample(N, model, n_per, SEED, *c["packets"][g], c["surface0"], trajectory_offset=c["offset"] + g * n_per)
            assert same_bits(plain, tuple(a[sl] for a in got)), g
        return
    # zero sigmas: the centre exactly, and b the column of C(x0): the bits the same call gives with only sigma_p positive, where x is x0 too
    assert np.array_equal(x, np.repeat(c["packets"][:, 0], n_per)) and np.array_equal(p, np.repeat(c["packets"][:, 1], n_per))
    mixed = c["packets"].copy()
    mixed[:, 3] = mixed[:, 1] / 20.0
    half = gpu.hop_sample_groups(N, model, n_per, SEED, mixed, c["surface0"])
    assert np.array_equal(half[0], x) and np.array_equal(half[2], b) and len(np.unique(half[1])) == c["n"]
    mixed[:, 2], mixed[:, 3] = 0.3, 0.0
    half = gpu.hop_sample_groups(N, model, n_per, SEED, mixed, c["surface0"])
    assert np.array_equal(half[1], p) and len(np.unique(half[0])) == c["n"]
    _, _, Cm, _ = HN.states(x, c["potential"])
    assert np.abs(np.abs(np.einsum("mik,mi->mk", Cm, b.real)) - np.eye(N)[c["surface0"]]).max() <= 1e-13


# ---- 2. evolve and observe: the plain calls on slices, bit for bit -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,shape", CASES)
def test_evolve_and_observe_bits(gpu, model_of, name, shape):
    c = case(name, shape)
    model, N, n_per, n, start = model_of(c), c["N"], c["n_per"], c["n"], c["start"]
    steps, cut = 400, 150
    grouped = lambda state, first, count, dt=c["dt"], **kw: gpu.hop_evolve_groups(N, model, state, n_per, SEED, MASS, dt, first, count, LEFT, RIGHT,
                                                                                   reverse=c["reverse"], trajectory_offset=c["offset"], **kw)
    zeros = np.zeros((n, 2), dtype=np.int32)
    whole, hops = grouped(start, 0, steps, hops=zeros)
    assert hops.dtype == np.int32 and hops.shape == (n, 2) and not zeros.any() and hops.min() >= 0
    assert same_bits(grouped(start, 0, steps), whole)                                   # hops = null: the same state bits
    again, hops2 = grouped(start, 0, steps, hops=zeros)
    assert same_bits(again, whole) and np.array_equal(hops2, hops)                      # a repeat
    first, part = grouped(start, 0, cut, hops=zeros)                                     # nothing hidden between two calls, hops accumulated
    second, both = grouped(first, cut, steps - cut, hops=part)
    assert same_bits(second, whole) and np.array_equal(both, hops)
    assert np.array_equal(grouped(start, 0, steps, hops=hops)[1], 2 * hops)              # added to what is there
    rows = gpu.hop_observe_groups(N, model, whole, n_per, MASS)
    assert rows.shape == (c["n_groups"], 4 * N + 3) and np.array_equal(gpu.hop_observe_groups(N, model, whole, n_per, MASS), rows)
    assert (rows[:, :3 * N].sum(axis=1) == n_per).all()
    for g, sl in enumerate(HS.slices(c["n_groups"], n_per)):                              # the plain calls on the slice
        plain = gpu.hop_evolve(N, model, tuple(a[sl] for a in start), SEED, MASS, c["dt"][g], 0, steps, LEFT, RIGHT, reverse=c["reverse"],
                               trajectory_offset=c["offset"] + g * n_per)
        assert same_bits(plain, tuple(a[sl] for a in whole)), g
        assert np.array_equal(gpu.hop_observe(N, model, plain, MASS), rows[g]), g
    assert (hops[:, 0] >= (whole[3] != start[3])).all()
    equal = np.full(c["n_groups"], 1.0)                                                   # all-equal dt: one plain call over the whole
    assert same_bits(grouped(start, 0, steps, dt=equal),
                     gpu.hop_evolve(N, model, start, SEED, MASS, 1.0, 0, steps, LEFT, RIGHT, reverse=c["reverse"], trajectory_offset=c["offset"]))
    dev = on_device(gpu, *start)                                                          # device pointers
    counters, = on_device(gpu, zeros)
    out, counted = grouped(dev, 0, steps, hops=counters)
    gpu.synchronize()
    assert all(o is d for o, d in zip(out, dev)) and counted is counters
    assert same_bits(tuple(t.cpu().numpy() for t in out), whole) and np.array_equal(counted.cpu().numpy(), hops)
    assert np.array_equal(gpu.hop_observe_groups(N, model, out, n_per, MASS), rows)
    done = whole[4] != 0                                                                  # a finished trajectory is frozen, its counters too
    later, more = grouped(whole, steps, 100, hops=hops)
    assert same_bits(tuple(a[done] for a in later), tuple(a[done] for a in whole)) and np.array_equal(more[done], hops[done])
    print(f"hop scan bits {name} {shape}: hops {hops[:, 0].sum()} frustrated {hops[:, 1].sum()} finished {done.sum()} of {n}")
    assert hops[:, 0].sum() >= 10, "the case tests nothing"


# ---- 3. the float64 restatement -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(name, shape):
    """The case on the restatement, once: evolved in float64 (with the counters and diagnostics) and in long double, and D per quantity"""
    assert np.finfo(np.longdouble).eps < 1e-18  # or D calibrates nothing
    c = case(name, shape)
    args = (c["n_per"], SEED, MASS, c["dt"], 0, c["steps"], LEFT, RIGHT, c["reverse"], c["offset"])
    end, hops, diag = HS.evolve_groups(c["potential"], c["start"], *args)
    wide, wide_hops, _ = HS.evolve_groups(c["potential"], widen(c["start"]), *args)
    assert np.array_equal(end[3], wide[3]) and np.array_equal(end[4], wide[4]) and np.array_equal(hops, wide_hops)
    return dict(end=end, hops=hops, diag=diag, D=[float(np.abs(end[q] - wide[q]).max()) for q in range(3)])


def test_against_the_restatement(gpu, model_of):
    name, shape = "dac-reverse", "5x67"  # every momentum of the issue's list, frustrated hops that reverse, a non-zero offset
    c, ref = case(name, shape), reference(name, shape)
    diag, (Dx, Dp, Db) = ref["diag"], ref["D"]
    keep = diag["margin"] >= 1e-10
    print(f"hop scan parity {name}: hops {ref['hops'][:, 0].sum()} frustrated {ref['hops'][:, 1].sum()} least margin {diag['margin'].min():.3g} "
          f"set aside {(~keep).sum()}; D x {Dx:.3g} p {Dp:.3g} b {Db:.3g}")
    assert keep.all(), "the restatement alone sets a trajectory aside: change the seed"
    assert ref["hops"][:, 0].sum() >= 10 and ref["hops"][:, 1].sum() >= 5, "the case tests nothing"
    got, hops = gpu.hop_evolve_groups(c["N"], model_of(c), c["start"], c["n_per"], SEED, MASS, c["dt"], 0, c["steps"], LEFT, RIGHT, reverse=c["reverse"],
                                      trajectory_offset=c["offset"], hops=np.zeros((c["n"], 2), dtype=np.int32))
    assert (~keep).sum() <= c["n"] // 100
    want = ref["end"]
    tol = [HN.tolerance(D, want[q]) for q, D in enumerate((Dx, Dp, Db))]
    err = [float(np.abs(got[q] - want[q])[keep].max()) for q in range(3)]
    print(f"hop scan parity {name}: err / tol x {err[0] / tol[0]:.3g} p {err[1] / tol[1]:.3g} b {err[2] / tol[2]:.3g}")
    assert np.array_equal(got[3][keep], want[3][keep]) and np.array_equal(got[4][keep], want[4][keep]) and np.array_equal(hops[keep], ref["hops"][keep])
    for q in range(3):
        assert err[q] <= tol[q], ("xpb"[q], err[q], tol[q])
    rows = gpu.hop_observe_groups(c["N"], c["model"], want, c["n_per"], MASS)  # the sums of the restatement's own end state
    terms = HN.observe_terms(c["potential"], want, MASS).reshape(c["n_groups"], c["n_per"], -1)
    assert np.array_equal(rows[:, :6], terms[:, :, :6].sum(axis=1))
    bound = c["n_per"] * EPS * np.abs(terms[:, :, 6:]).sum(axis=1)
    assert (np.abs(rows[:, 6:] - terms[:, :, 6:].sum(axis=1)) <= bound).all()


# ---- 4. GPLE_ERR_BAD_ARG --------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments(gpu):
    c = case("dac", "5x67")
    lib, ctx, n = gpu.lib, gpu.ctx, c["n"]
    x, p, b, surface, status = (a.copy() for a in c["start"])
    hops, out = np.full((n, 2), 7, dtype=np.int32), np.full((5, 11), -1.0)
    before = tuple(a.copy() for a in (x, p, b, surface, status, hops, out))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    arrays = dict(x=x.ctypes.data_as(dp), p=p.ctypes.data_as(dp), b=b.ctypes.data_as(dp), surface=surface.ctypes.data_as(ip), status=status.ctypes.data_as(ip))
    nan, inf = float("nan"), float("inf")
    tables = []  # keeps the tables of the calls alive

    def table(values):
        tables.append(np.ascontiguousarray(values, dtype=np.float64))
        return tables[-1].ctypes.data_as(dp)

    def packets(at=None):
        t = c["packets"].copy()
        for (g, k), v in (at or {}).items():
            t[g, k] = v
        return table(t)

    def sample(**kw):
        a = dict(num_pes=2, model=1, groups=5, per=67, offset=0, seed=1, packets=packets(), surface0=0, flags=0, **arrays)
        a.update(kw)
        return lib.gple_hop_sample_groups(ctx, a["num_pes"], a["model"], a["groups"], a["per"], a["offset"], a["seed"], a["packets"], a["surface0"], a["flags"],
                                          a["x"], a["p"], a["b"], a["surface"], a["status"])

    def evolve(**kw):
        a = dict(num_pes=2, model=1, groups=5, per=67, offset=0, seed=1, mass=MASS, dt=table(c["dt"]), first=0, steps=3, left=LEFT, right=RIGHT, flags=0,
                 hops=hops.ctypes.data_as(ip), **arrays)
        a.update(kw)
        return lib.gple_hop_evolve_groups(ctx, a["num_pes"], a["model"], a["groups"], a["per"], a["offset"], a["seed"], a["mass"], a["dt"], a["first"], a["steps"],
                                          a["left"], a["right"], a["flags"], a["x"], a["p"], a["b"], a["surface"], a["status"], a["hops"])

    def observe(**kw):
        a = dict(num_pes=2, model=1, groups=5, per=67, mass=MASS, flags=0, out=out.ctypes.data_as(dp), **arrays)
        a.update(kw)
        return lib.gple_hop_observe_groups(ctx, a["num_pes"], a["model"], a["groups"], a["per"], a["mass"], a["flags"], a["x"], a["p"], a["b"], a["surface"],
                                           a["status"], a["out"])

    shared = [dict(num_pes=1), dict(num_pes=4), dict(model=-1), dict(model=3), dict(model=7), dict(model=_capi.PES_USER + 15), dict(groups=0), dict(per=0),
              dict(groups=_capi.HOP_MAX_GROUPS + 1, per=1), dict(groups=65536, per=1 << 60), dict(groups=5, per=(1 << 64) // 5 + 1),
              dict(groups=4, per=(1 << 30) + 1)] + [{k: None} for k in arrays]
    beyond = [dict(offset=LAST - n + 1)]
    for kw in shared + beyond + [dict(surface0=-1), dict(surface0=2), dict(packets=None)] + [
            dict(packets=packets(at={(g, k): v})) for g, k, v in ((0, 0, nan), (4, 0, inf), (2, 1, nan), (4, 1, -inf), (1, 2, -1.0), (4, 2, nan), (0, 2, inf),
                                                                   (3, 3, -1e-300), (4, 3, nan), (2, 3, inf))]:
        assert sample(**kw) == BAD_ARG, kw
    for kw in shared + beyond + [dict(mass=0.0), dict(mass=-1.0), dict(mass=nan), dict(mass=inf), dict(left=RIGHT), dict(left=7.0), dict(left=nan), dict(right=nan),
                                 dict(steps=(1 << 40) + 1), dict(dt=None)] + [dict(dt=table(np.where(np.arange(5) == g, v, c["dt"])))
                                                                              for g, v in ((0, 0.0), (4, -1.0), (2, nan), (4, inf))]:
        assert evolve(**kw) == BAD_ARG, kw
    for kw in shared + [dict(mass=0.0), dict(mass=nan), dict(mass=inf), dict(out=None)]:
        assert observe(**kw) == BAD_ARG, kw
    assert same_bits((x, p, b, surface, status, hops, out), before)  # a refused call writes nothing
    # what is not refused: the last admissible offset, zero sigmas, a null hops, no step at all
    assert evolve(offset=LAST - n, hops=None) == 0 and np.array_equal(hops, before[5]) and not np.array_equal(x, before[0])
    x[:] = before[0]
    assert evolve(steps=0) == 0 and np.array_equal(x, before[0]) and np.array_equal(hops, before[5])
    assert sample(packets=packets(at={(0, 2): 0.0, (0, 3): 0.0}), offset=LAST - n) == 0 and (x[:67] == X0).all() and (p[:67] == 8.0).all()
    assert observe() == 0 and out[:, :6].sum() == n


# ---- 5. the driver ---------------------------------------------------------------------------------------------------------------------------------
def test_driver_against_the_same_scan_on_the_restatement(gpu, tmp_path):
    kw = dict(model=hopping.DAC, num_pes=2, momenta=[10.0, 16.0, 30.0], n_per_group=128, seed=SEED, dt=[2.0, 1.0, 1.0], chunk_steps=256, x0=X0, xmin=LEFT,
              xmax=RIGHT)
    res = hopping.scan(gpu, out_dir=str(tmp_path), **kw)
    api = HS.NumpyScanApi()
    ref = hopping.scan(api, **kw)
    assert hasattr(res["state"][0], "is_cuda") and res["state"][0].is_cuda and res["hop_counts"].is_cuda  # the ensemble stayed on the device
    assert res["stop"] is not None and res["stop"] == ref["stop"] and res["steps"] == ref["steps"] > 0
    assert (res["state"][0].cpu().numpy() != X0).all()
    assert np.array_equal(res["rows"][:, :6], ref["rows"][:, :6]) and np.array_equal(res["scattered"], ref["scattered"]) and not res["running"].any()
    assert np.array_equal(res["hop_counts"].cpu().numpy(), ref["hop_counts"]) and np.array_equal(res["hops"], ref["hops"]) and res["hops"].sum() > 0
    assert np.array_equal(res["stderr"], ref["stderr"]) and np.array_equal(res["head"], ref["head"])
    terms = HN.observe_terms(HN.builtin(HN.DAC, 2), ref["state"], MASS).reshape(3, 128, -1)
    bound = 128 * EPS * np.abs(terms[:, :, 6:]).sum(axis=1)  # the observe tolerance of DESIGN.md §17, per group
    err = np.abs(res["rows"][:, 6:] - ref["rows"][:, 6:])
    print(f"hop scan driver: {res['steps']} steps, hops {res['hops']}, frustrated {res['frustrated']}; sums err / tol {np.max(err / bound):.3g}")
    assert (err <= bound).all()
    assert np.abs(res["energy_drift"] - ref["energy_drift"]).max() <= 2.0 * bound[:, -1].max() / 128
    lines = [[float(v) for v in line.split()] for line in open(tmp_path / "scan.txt")]
    assert len(lines) == 3 and all(len(line) == 14 for line in lines)
    for g, line in enumerate(lines):
        f = [*res["scattered"][g].reshape(-1), res["running"][g]]
        want = [res["head"][g], *f, *res["stderr"][g], res["hops"][g], res["frustrated"][g], res["energy_drift"][g]]
        assert np.allclose(line, want, rtol=1e-5, atol=1e-300) and abs(sum(f) - 1.0) < 1e-12
    # the result does not depend on the chunk, bit for bit
    other = hopping.scan(gpu, **{**kw, "chunk_steps": 100, "max_steps": res["steps"]})
    assert same_bits(tuple(t.cpu().numpy() for t in other["state"]), tuple(t.cpu().numpy() for t in res["state"]))
    assert np.array_equal(other["hop_counts"].cpu().numpy(), res["hop_counts"].cpu().numpy()) and np.array_equal(other["rows"], res["rows"])
