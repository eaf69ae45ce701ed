"""GPU: the absorbing boundary of the exact MQCLE run (gple_mqcl_absorb, gple_mqcl_evolve_absorbing; csrc/gple_mqcl_absorb.hip; DESIGN.md §12,
"The absorbing boundary") against the numpy restatement tests/mqcl_absorbing_numpy.py, and the driver exact_mqcl.run(boundary=ABSORBING)
against a numpy run of its loop.  Every test needs the feature (the entry points and the `boundary` argument)."""
import ctypes as C

import numpy as np
import pytest

from gaussian_process_liouville_equation_amd import exact
from gaussian_process_liouville_equation_amd import exact_mqcl as EM
from tests import mqcl_absorbing_numpy as MA
from tests import mqcl_numpy as MN
from tests import pes_table_numpy as PT
from tests import test_gpu_mqcl as TM

pytestmark = pytest.mark.gpu
BAD_ARG = 1
EVOLVE_TOL = TM.EVOLVE_TOL  # the propagator's own distance from its restatement, relative to max|rho|
BOOK_TOL = 1e-13            # per booked entry g_i rho^adia_aa and row, relative to max|rho|: the bound of the observe tests on the adiabatic rho


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64).ravel()


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


@pytest.fixture
def define(gpu, monkeypatch):
    """define(table) -> model id on the session's context, with the restatement patched to see the table under that id; undefined at the end"""
    ids, tables = [], {}
    PT.install(monkeypatch, tables)

    def make(table):
        model = gpu.pes_define(table.num_pes, *table.args())
        ids.append(model)
        tables[model] = table
        return model

    yield make
    for model in ids:
        gpu.pes_undefine(model)


def user_table(num_pes):
    return PT.function_table(PT.other_dac if num_pes == 2 else PT.three_level, -14.0, 14.0, 0.125)


def flat_table():
    return PT.Table(-1.0, 2.0, np.tile(np.diag(MA.FLAT_LEVELS), (2, 1, 1)), np.zeros((2, 2, 2)))


def random_mask(n, rng):
    """g on a random third of the rows (two at least), an exact 1 and an exact 0 among the chosen values"""
    rows = rng.choice(n, max(2, n // 3), replace=False)
    g = np.zeros(n)
    g[rows] = rng.uniform(0.0, 1.0, len(rows))
    g[rows[0]], g[rows[1]] = 1.0, 0.0
    return g


def book_bound(g, n_left, scale, masks=1):
    """per side: BOOK_TOL max|rho| times the absorbing rows on that side, times the number of masks"""
    live = np.flatnonzero(g != 0.0)
    return np.array([np.sum(live < n_left), np.sum(live >= n_left)]) * (BOOK_TOL * scale * masks)


def book_check(what, dev, ref, bound):
    for side in (0, 1):
        err = np.abs(dev[side] - ref[side]).max()
        print(f"{what} side {side}: measured {err:.3g} / bound {bound[side]:.3g}")
        assert err <= bound[side], (what, side, err, bound[side])


def model_of(name, num_pes, define):
    return {"sac": 0, "dac": 1, "tsac": 3}[name] if name != "table" else define(user_table(num_pes))


# ---- 1. one mask -----------------------------------------------------------------------------------------------------------------------------
# n: a row shorter than a wave (5), ragged tails (33, 129, 300), a full trip of the 256-strided loop and its second and third (257, 300, 1025),
# the smallest grid of the NT = 512 family of the propagator (1025)
@pytest.mark.parametrize("num_pes, name, n", [(2, "sac", n) for n in (5, 33, 64, 129, 257, 300, 1025)] + [(2, "table", 33), (2, "table", 257),
                                                                                                          (3, "tsac", 33), (3, "tsac", 257), (3, "table", 33)])
def test_absorb_against_restatement(gpu, define, num_pes, name, n):
    import torch

    model = model_of(name, num_pes, define)
    rng = np.random.default_rng(1000 * num_pes + n)
    x = TM.grid(n)[0]
    rho = MN.random_hermitian(num_pes, n, rng)
    g = random_mask(n, rng)
    bases = MN.Bases(x, model, num_pes)
    scale = np.abs(rho).max()
    want = (1.0 - g)[None, None, :, None, None] * rho.view(np.float64).reshape(num_pes, num_pes, n, n, 2)
    for n_left in (0, n // 3, n):
        ref_rho, ref_sums = MA.absorb(rho, bases, g, n_left)
        out, acc = gpu.mqcl_absorb(num_pes, model, x, rho, g, n_left)
        assert same_bits(out, want) and same_bits(out, ref_rho)
        assert same_bits(out[:, :, g == 0.0], rho[:, :, g == 0.0])
        assert np.array_equal(out, np.conj(np.swapaxes(out, 0, 1))) and all((out[a, a].imag == 0.0).all() for a in range(num_pes))
        book_check(f"absorb num_pes {num_pes} {name} n {n} n_left {n_left}", acc, ref_sums, book_bound(g, n_left, scale))
        # onto a non-zero accumulator: one addition per entry
        start = rng.standard_normal((2, num_pes, n))
        out2, acc2 = gpu.mqcl_absorb(num_pes, model, x, rho, g, n_left, start)
        assert same_bits(acc2, start + acc) and same_bits(out2, out)
        # device pointers: the same bits, in place
        tx, tg, tr, ta = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (x, g, rho, start))
        torch.cuda.synchronize()
        r_dev, a_dev = gpu.mqcl_absorb(num_pes, model, tx, tr, tg, n_left, ta)
        gpu.synchronize()
        assert r_dev is tr and a_dev is ta and same_bits(tr.cpu().numpy(), out) and same_bits(ta.cpu().numpy(), acc2)


def test_absorb_without_an_absorbing_row_changes_nothing(gpu):
    n = 33
    x = TM.grid(n)[0]
    rho = MN.random_hermitian(2, n, np.random.default_rng(0))
    start = np.random.default_rng(1).standard_normal((2, 2, n))
    out, acc = gpu.mqcl_absorb(2, 1, x, rho, np.zeros(n), 10, start)
    assert same_bits(out, rho) and same_bits(acc, start)


# ---- 2. the blocks against the separate calls ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_pes, model, n, mask_every, steps", [(2, 1, 129, 1, 6), (2, 1, 129, 3, 6), (3, 3, 257, 2, 4)])
def test_evolve_absorbing_is_the_sequence_of_separate_calls(gpu, num_pes, model, n, mask_every, steps):
    import torch

    rng = np.random.default_rng(n + mask_every)
    x, p, lx, lp = TM.grid(n)
    rho = MN.random_hermitian(num_pes, n, rng)
    g, n_left = random_mask(n, rng), n // 2
    start = rng.standard_normal((2, num_pes, n))
    out, acc = gpu.mqcl_evolve_absorbing(num_pes, model, x, p, rho, 2000.0, lx, lp, 0.25, steps, mask_every, g, n_left, start)
    r, a = rho, start
    for _ in range(steps // mask_every):
        r, a = gpu.mqcl_absorb(num_pes, model, x, r, g, n_left, a)
        r = gpu.mqcl_evolve(num_pes, model, x, p, r, 2000.0, lx, lp, 0.25, mask_every)
        r, a = gpu.mqcl_absorb(num_pes, model, x, r, g, n_left, a)
    assert same_bits(out, r) and same_bits(acc, a)
    assert not same_bits(out, gpu.mqcl_evolve(num_pes, model, x, p, rho, 2000.0, lx, lp, 0.25, steps))
    # repeats and device pointers
    out2, acc2 = gpu.mqcl_evolve_absorbing(num_pes, model, x, p, rho, 2000.0, lx, lp, 0.25, steps, mask_every, g, n_left, start)
    assert same_bits(out2, out) and same_bits(acc2, acc)
    tx, tp, tg, tr, ta = (torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (x, p, g, rho, start))
    torch.cuda.synchronize()
    gpu.mqcl_evolve_absorbing(num_pes, model, tx, tp, tr, 2000.0, lx, lp, 0.25, steps, mask_every, tg, n_left, ta)
    gpu.synchronize()
    assert same_bits(tr.cpu().numpy(), out) and same_bits(ta.cpu().numpy(), acc)


# ---- 3. the blocks against the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_pes, model", [(2, 1), (3, 3)])
@pytest.mark.parametrize("n", [64, 100, 127])
def test_evolve_absorbing_against_restatement(gpu, num_pes, model, n):
    rng = np.random.default_rng(10 * n + num_pes)
    x, p, lx, lp = TM.grid(n)
    rho = MN.random_hermitian(num_pes, n, rng)
    g, n_left = random_mask(n, rng), n // 2
    steps, mask_every = 12, 4
    out, acc = gpu.mqcl_evolve_absorbing(num_pes, model, x, p, rho, 2000.0, lx, lp, 0.25, steps, mask_every, g, n_left)
    ref, ref_acc = MA.evolve_absorbing(rho, MN.Bases(x, model, num_pes), p, 2000.0, lx, lp, 0.25, steps, mask_every, g, n_left)
    d = np.abs(out - ref).max() / np.abs(ref).max()
    print(f"evolve_absorbing num_pes {num_pes} n {n}: state {d:.3g} / {EVOLVE_TOL:.3g}")
    assert d <= EVOLVE_TOL
    assert np.array_equal(out, np.conj(np.swapaxes(out, 0, 1)))
    book_check(f"evolve_absorbing num_pes {num_pes} n {n}", acc, ref_acc, book_bound(g, n_left, np.abs(rho).max(), masks=2 * steps // mask_every))


# ---- 4., 5. the two cases of the CPU tests on the device ---------------------------------------------------------------------------------------
def case_on_device(gpu, model, case, steps, mask_every):
    """max|rho| of the state's bound is the largest magnitude the run handles, the initial state's: a mask only shrinks the state (0 <= 1 - g <= 1)
    and the propagator moves it, so the rounding of every step is relative to that.  A run that empties the box keeps that noise while its own
    maximum goes: free flight leaves 1.5e-6 of the initial maximum, and the restatement's own final state moves by 1.4e-9 of its final maximum
    (2e-15 of the initial one) when the start is perturbed by one ulp.  The figure relative to the final maximum is printed beside it."""
    G, bases, rho0, ref, ref_acc = case
    out, acc = gpu.mqcl_evolve_absorbing(2, model, G["x"], G["p"], rho0, G["mass"], G["length_x"], G["length_p"], G["dt"], steps, mask_every, G["g"], G["n_left"])
    d = np.abs(out - ref).max() / np.abs(rho0).max()
    print(f"state {d:.3g} / {EVOLVE_TOL:.3g} of the initial maximum ({np.abs(out - ref).max() / np.abs(ref).max():.3g} of the final one, "
          f"which is {np.abs(ref).max() / np.abs(rho0).max():.3g} of the initial)")
    assert d <= EVOLVE_TOL
    bound = book_bound(G["g"], G["n_left"], np.abs(rho0).max(), masks=2 * steps // mask_every)
    book_check("accumulator", acc, ref_acc, bound)
    w = G["dx"] * G["dp"]
    figures, ref_figures = acc.sum(axis=2) * w, ref_acc.sum(axis=2) * w
    assert (np.abs(figures - ref_figures) <= bound[:, None] * G["n"] * w).all()
    _, _, pops = gpu.mqcl_observe(2, model, G["x"], G["p"], out, G["mass"], G["dx"], G["dp"])
    balance = figures.sum() + pops.sum() - 1.0
    print(f"absorbed {figures.ravel()}, inside {pops}, balance {balance:.3g}")
    assert abs(balance) <= 1e-11
    return figures, pops


def test_sac_case_on_the_device(gpu):
    figures, pops = case_on_device(gpu, 0, MA.sac_case(), 200, 8)
    assert figures[1, 0] > 0.1


def test_free_flight_on_a_flat_user_table(gpu, define):
    figures, pops = case_on_device(gpu, define(flat_table()), MA.free_flight_case(), 300, 1)
    assert figures[1, 0] > 0.99 and abs(pops.sum()) < 1e-3


# ---- 6. arguments ----------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_leave_state_and_accumulator_alone(gpu):
    lib, ctx = gpu.lib, gpu.ctx
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    n = 16
    x, p = TM.grid(n)[:2]
    rng = np.random.default_rng(6)
    g = random_mask(n, rng)
    rho = MN.random_hermitian(2, n, rng)
    acc = rng.standard_normal((2, 2, n))
    rho0, acc0 = rho.copy(), acc.copy()
    px, pp, pg, pr, pa = ptr(x), ptr(p), ptr(g), ptr(rho), ptr(acc)
    ab = lambda num_pes=2, model=1, x=px, n=n, g=pg, n_left=5, rho=pr, acc=pa: lib.gple_mqcl_absorb(ctx, num_pes, model, x, n, g, n_left, 0, rho, acc)
    for bad in (dict(num_pes=4), dict(num_pes=1), dict(model=3), dict(model=7), dict(model=-1), dict(n=3), dict(n=4097), dict(n_left=n + 1),
                dict(x=None), dict(g=None), dict(rho=None), dict(acc=None)):
        assert ab(**bad) == BAD_ARG, bad
    assert lib.gple_mqcl_absorb(None, 2, 1, px, n, pg, 5, 0, pr, pa) == BAD_ARG

    def ev(num_pes=2, model=1, x=px, p=pp, n=n, mass=2000.0, lx=20.0, lp=80.0, dt=0.25, steps=6, mask_every=3, g=pg, n_left=5, rho=pr, acc=pa):
        return lib.gple_mqcl_evolve_absorbing(ctx, num_pes, model, x, p, n, mass, lx, lp, dt, steps, mask_every, g, n_left, 0, rho, acc)

    for bad in (dict(num_pes=4), dict(model=3), dict(model=7), dict(n=3), dict(n=4097), dict(n_left=n + 1), dict(mask_every=0), dict(mask_every=4),
                dict(mask_every=7), dict(x=None), dict(p=None), dict(g=None), dict(rho=None), dict(acc=None), dict(mass=0.0), dict(mass=-1.0),
                dict(mass=float("inf")), dict(lx=0.0), dict(lp=float("nan")), dict(dt=float("nan")), dict(steps=(1 << 40) + 3)):
        assert ev(**bad) == BAD_ARG, bad
    assert same_bits(rho, rho0) and same_bits(acc, acc0)
    # and the same arguments without the mistake are accepted; no steps: nothing happens
    assert ev(steps=0) == 0 and same_bits(rho, rho0) and same_bits(acc, acc0)
    assert ev() == 0 and ab() == 0
    assert not same_bits(rho, rho0) and not same_bits(acc, acc0)


# ---- 7. the driver ---------------------------------------------------------------------------------------------------------------------------
def test_driver_run_matches_numpy_loop(gpu, tmp_path):
    """SAC from x0 = 8 (the packet's tail already in the right-hand absorber) on a coarse grid: box [-9.375, 9.375], dx = 1/8, 5 absorber rows a
    side, n = 161; dt = 2, 16 steps per output, a mask pair every 8 by the rule (0.125 / (11.5 / 2000 * 2) = 10.9); 4 outputs"""
    kw = dict(mass=2000.0, x0=8.0, xmin=-9.375, xmax=9.375, p0=10.0, sigma_p=0.5, dx=0.125, dt=2.0, output_time=32.0)
    res = EM.run(gpu, model=0, num_pes=2, boundary=exact.ABSORBING, until_absorbed=True, max_outputs=4, out_dir=str(tmp_path), write_phase="text", **kw)
    s = res["setup"]
    G = MA.grid(-9.375, 9.375, 0.125, 10.0, 0.5, 2000.0, 8, 2.0)
    assert (s["n_grids"], s["n_absorbing"], s["mask_every"], s["output_step"], s["n_left"]) == (161, 5, 8, 16, G["n_left"])
    assert np.array_equal(s["x"], G["x"]) and np.array_equal(s["p"], G["p"]) and np.array_equal(s["g"], G["g"]) and s["length_x"] == G["length_x"]
    bases = MN.Bases(G["x"], 0, 2)
    rho0 = MN.transform(EM.initial_density(G["x"], G["p"], G["dx"], G["dp"], 8.0, 10.0, G["sigma_x"], 0.5, 2), bases, MN.ADIABATIC, MN.DIABATIC)
    ref, stop, ref_rho, ref_acc = MA.run(rho0, bases, G, 4, 16, 8.0, until_absorbed=True)
    records = res["records"]
    assert stop is None and not res["stopped"] and len(records) == 5 and records[0]["t"] == 0.0 and not records[0]["absorbed"].any()
    for got, want in zip(records[1:], ref):
        assert got["t"] == want["t"]
        av = np.array([want["E"], want["x"], want["p"]])
        assert np.abs(np.array([got["E"], got["x"], got["p"]]) - av).max() <= 1e-10 * np.abs(av).max()
        assert np.abs(got["populations"] - want["populations"]).max() <= 1e-10 and np.abs(got["absorbed"] - want["absorbed"]).max() <= 1e-10
        assert abs(got["absorbed"].sum() + got["populations"].sum() - 1.0) <= 1e-11
    assert records[-1]["absorbed"][1, 0] > 0.05
    assert np.abs(res["absorbed_p"] - ref_acc * G["dx"]).max() <= 1e-10 * np.abs(ref_acc * G["dx"]).max()
    assert np.abs(res["rho"].cpu().numpy() - ref_rho).max() <= EVOLVE_TOL * np.abs(ref_rho).max()
    # the files parse back to the returned values at %g
    at_g = lambda values: [float("%g" % v) for v in np.ravel(values)]
    lines = [[float(v) for v in line.split()] for line in open(tmp_path / "absorbed.txt").read().splitlines()]
    assert len(lines) == 5 and all(line == at_g([r["t"], *r["absorbed"].ravel(), r["populations"].sum()]) for line, r in zip(lines, records))
    lines = [[float(v) for v in line.split()] for line in open(tmp_path / "absorbed_p.txt").read().splitlines()]
    assert len(lines) == 4 and all(line == at_g(row) for line, row in zip(lines, res["absorbed_p"].reshape(4, 161)))
    assert np.array_equal(np.loadtxt(tmp_path / "t.txt"), at_g([r["t"] for r in records]))
    avg = np.loadtxt(tmp_path / "averages.txt")
    assert np.array_equal(avg, np.array([at_g([r["t"], r["E"], r["x"], r["p"], *r["populations"]]) for r in records]))
    blocks = open(tmp_path / "phase.txt").read().split("\n\n")
    assert len([b for b in blocks if b.strip()]) == 5
    last = records[-1]
    assert res["scattering_line"] == " ".join("%g" % v for v in [s["p0"], *last["absorbed"].ravel(), last["populations"].sum()])
    assert res["final_line"] == " ".join("%g" % v for v in [s["p0"], *last["populations"]])
