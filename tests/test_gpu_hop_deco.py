"""GPU: surface hopping with the decoherence correction 6a (gple_hop_evolve_dc / gple_hop_evolve_groups_dc, csrc/gple_hop.hip; DESIGN.md §17,
"Decoherence corrections") against the numpy restatement tests/hop_deco_numpy.py, trajectory by trajectory.

The constants, cases and start ensembles are those of tests/test_gpu_hop.py (293 trajectories, seed 20250117, x0 = -4, sigma_p = p0 / 20,
sigma_x = 1 / (2 sigma_p), mass 2000, bounds +-6), edc_c = 0.1 throughout.  The rule is §17's own: surface, status and both hop counters must
be EQUAL to the float64 restatement's; x, p, b lie within 64 D_q + 1e-13 max(1, max|q|), D_q being the largest distance between the float64 and
the long double restatement of that case and mode, computed here.  A trajectory is set aside only where the float64 restatement's own margin
|xi - (g_1 + ... + g_k)| is below 1e-10, at most 2 of 293 may be, and that cap and the agreement of the two restatements' decisions are asserted
before the device is asked.  The hop counters come from the grouped call (one group), whose state must have the bits of the plain call's.  The
ratios measured on the MI355X are in DESIGN.md §17."""
import ctypes as C
import functools

import numpy as np
import pytest

from gaussian_process_liouville_equation_amd import _capi, hopping
from tests import hop_deco_numpy as HD
from tests import hop_density_numpy as HB
from tests import hop_numpy as HN
from tests import hop_scan_numpy as HS
from tests.test_gpu_hop import LEFT, MASS, N_TRAJ, RIGHT, SEED, X0, model_of, same_bits, widen  # noqa: F401  (model_of is a fixture)
from tests.test_gpu_hop import reference as plain_reference

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
EDC_C = 0.1
BAD_ARG = 1
NAMES = {HD.NONE: "none", HD.EDC: "edc", HD.COLLAPSE_HOP: "collapse_hop", HD.COLLAPSE_ATTEMPT: "collapse_attempt"}

# name: the case of tests/test_gpu_hop.py (model, p0, dt, steps, start surface, GPLE_HOP_REVERSE) and the mode
CASES = {
    "dac10-edc": ("dac10", HD.EDC),
    "dac10-collapse_hop": ("dac10", HD.COLLAPSE_HOP),
    "dac10-reverse-collapse_attempt": ("dac10-reverse", HD.COLLAPSE_ATTEMPT),
    "dac16-edc": ("dac16", HD.EDC),
    "ecr-edc": ("ecr", HD.EDC),
    "ecr-collapse_hop": ("ecr", HD.COLLAPSE_HOP),
    "tsac-edc": ("tsac", HD.EDC),
    "tsac-collapse_hop": ("tsac", HD.COLLAPSE_HOP),
    "table3-edc": ("table3", HD.EDC),
}


@functools.lru_cache(maxsize=None)
def reference(name):
    """The case on the restatement, once: its evolution with the correction in float64 (with diagnostics) and in long double, D per quantity,
    and the preconditions of the comparison.  The start ensemble and the uncorrected end state are tests/test_gpu_hop.py's own"""
    assert np.finfo(np.longdouble).eps < 1e-18  # or D calibrates nothing
    plain_name, mode = CASES[name]
    base = plain_reference(plain_name)
    c, pot, start = base["case"], base["potential"], base["start"]
    args = (SEED, MASS, c["dt"], 0, c["steps"], LEFT, RIGHT)
    end, diag = HD.evolve(pot, start, *args, reverse=c["reverse"], decoherence=mode, edc_c=EDC_C)
    wide, _ = HD.evolve(pot, widen(start), *args, reverse=c["reverse"], decoherence=mode, edc_c=EDC_C)
    keep = diag["margin"] >= 1e-10
    assert (~keep).sum() <= 2, "the restatement alone sets too many aside"
    assert np.array_equal(end[3][keep], wide[3][keep]) and np.array_equal(end[4][keep], wide[4][keep])
    D = [float(np.abs(end[q] - wide[q])[keep].max()) for q in range(3)]
    # the case tests something: hops, and an end state that is not the uncorrected one
    none = base["end"]
    assert diag["hops"].sum() >= 10, "the case tests nothing"
    moved = int(((end[3] != none[3]) | (end[4] != none[4])).sum())
    b_moved = float(np.abs(end[2] - none[2]).max())
    assert moved > 0 or b_moved > 0.1, "the correction changes nothing"
    return dict(case=c, mode=mode, potential=pot, start=start, end=end, diag=diag, D=D, keep=keep, moved=moved, b_moved=b_moved)


def evolve_plain(gpu, c, model, state, first, steps, mode, edc_c=EDC_C, **kw):
    return gpu.hop_evolve(c["N"], model, state, SEED, MASS, c["dt"], first, steps, LEFT, RIGHT, reverse=c["reverse"], decoherence=mode, edc_c=edc_c, **kw)


def evolve_counted(gpu, c, model, state, first, steps, mode, hops=None, edc_c=EDC_C):
    """the grouped call over one group of the whole ensemble -> (state, hops)"""
    hops = np.zeros((len(state[0]), 2), dtype=np.int32) if hops is None else hops
    return gpu.hop_evolve_groups(c["N"], model, state, len(state[0]), SEED, MASS, [c["dt"]], first, steps, LEFT, RIGHT, reverse=c["reverse"], hops=hops,
                                 decoherence=mode, edc_c=edc_c)


# ---- 1. parity per trajectory ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_parity_per_trajectory(gpu, model_of, name):
    ref = reference(name)  # every precondition is asserted in there, on the host
    c, mode, diag, keep, (Dx, Dp, Db) = ref["case"], ref["mode"], ref["diag"], ref["keep"], ref["D"]
    model = model_of(c)
    got, hops = evolve_counted(gpu, c, model, ref["start"], 0, c["steps"], mode)  # one launch: the state never leaves the registers
    assert same_bits(evolve_plain(gpu, c, model, ref["start"], 0, c["steps"], NAMES[mode]), got)  # the plain kernel, the mode by its name
    want = ref["end"]
    tol = [HN.tolerance(D, want[q]) for q, D in enumerate((Dx, Dp, Db))]
    err = [float(np.abs(got[q] - want[q])[keep].max()) for q in range(3)]
    print(f"hop deco parity {name}: hops {diag['hops'].sum()} frustrated {diag['frustrated'].sum()} least margin {diag['margin'].min():.3g} "
          f"set aside {(~keep).sum()}; differs from no correction in {ref['moved']} decisions, b by {ref['b_moved']:.3g}; "
          f"D x {Dx:.3g} p {Dp:.3g} b {Db:.3g}; err / tol x {err[0] / tol[0]:.3g} p {err[1] / tol[1]:.3g} b {err[2] / tol[2]:.3g}")
    assert np.array_equal(got[3][keep], want[3][keep]) and np.array_equal(got[4][keep], want[4][keep])
    assert np.array_equal(hops[keep, 0], diag["hops"][keep]) and np.array_equal(hops[keep, 1], diag["frustrated"][keep])
    for q in range(3):
        assert err[q] <= tol[q], (name, "xpb"[q], err[q], tol[q])


# ---- 2. bits ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plain_name", ["dac10", "table3"])
def test_bits(gpu, model_of, plain_name):
    import torch

    base = plain_reference(plain_name)
    c, start = base["case"], base["start"]
    model = model_of(c)
    steps, cut = 400, 150
    # GPLE_HOP_DC_NONE through both new entry points: the old entry points' bits
    old = gpu.hop_evolve(c["N"], model, start, SEED, MASS, c["dt"], 0, steps, LEFT, RIGHT, reverse=c["reverse"])
    assert same_bits(evolve_plain(gpu, c, model, start, 0, steps, "none"), old) and same_bits(evolve_plain(gpu, c, model, start, 0, steps, HD.NONE, edc_c=-1.0), old)
    zeros = np.zeros((N_TRAJ, 2), dtype=np.int32)
    old_grouped = gpu.hop_evolve_groups(c["N"], model, start, N_TRAJ, SEED, MASS, [c["dt"]], 0, steps, LEFT, RIGHT, reverse=c["reverse"], hops=zeros)
    new_grouped = evolve_counted(gpu, c, model, start, 0, steps, "none")
    assert same_bits(new_grouped[0], old) and same_bits(old_grouped[0], old) and np.array_equal(new_grouped[1], old_grouped[1])
    ends = {}
    for mode in (HD.EDC, HD.COLLAPSE_HOP, HD.COLLAPSE_ATTEMPT):
        whole = ends[mode] = evolve_plain(gpu, c, model, start, 0, steps, mode)
        assert not same_bits(whole, old)                                                                              # the mode reaches the kernel
        assert same_bits(evolve_plain(gpu, c, model, evolve_plain(gpu, c, model, start, 0, cut, mode), cut, steps - cut, mode), whole)  # nothing hidden
        assert same_bits(evolve_plain(gpu, c, model, start, 0, steps, mode), whole)                                   # a repeat
        part = evolve_plain(gpu, c, model, tuple(a[100:] for a in start), 0, steps, mode, trajectory_offset=100)      # a slice with its offset
        assert same_bits(part, tuple(a[100:] for a in whole))
        other = evolve_plain(gpu, c, model, start, 0, steps, mode, edc_c=0.02)                                        # edc_c is read in mode EDC only
        assert same_bits(other, whole) == (mode != HD.EDC)
        where = torch.device("cuda", gpu.device)                                                                       # device pointers
        on_device = tuple(torch.from_numpy(a.copy()).to(where) for a in start)
        torch.cuda.synchronize(where)
        out = evolve_plain(gpu, c, model, on_device, 0, steps, mode)
        gpu.synchronize()
        assert all(o is d for o, d in zip(out, on_device)) and same_bits(tuple(t.cpu().numpy() for t in out), whole)
        counted, hops = evolve_counted(gpu, c, model, start, 0, steps, mode)                                           # the grouped kernel, one group
        assert same_bits(counted, whole) and hops[:, 0].sum() >= 5
        if plain_name == "dac10":
            done = whole[4] != 0                                                                                      # a finished trajectory is frozen
            assert done.any()
            later = evolve_plain(gpu, c, model, whole, steps, 200, mode)
            assert same_bits(tuple(a[done] for a in later), tuple(a[done] for a in whole))
    assert not same_bits(ends[HD.COLLAPSE_HOP], ends[HD.EDC])
    if plain_name == "dac10":  # frustrated hops: the two collapse modes differ from each other
        far = {mode: evolve_plain(gpu, c, model, start, 0, c["steps"], mode) for mode in (HD.COLLAPSE_HOP, HD.COLLAPSE_ATTEMPT)}
        assert not same_bits(far[HD.COLLAPSE_HOP], far[HD.COLLAPSE_ATTEMPT])


@pytest.mark.parametrize("mode", [HD.EDC, HD.COLLAPSE_HOP, HD.COLLAPSE_ATTEMPT])
def test_grouped_against_plain_per_slice(gpu, mode):
    """5 x 67 trajectories (group edges inside waves and inside a workgroup) with mixed dt: tests/test_gpu_hop_scan.py's reversing DAC case"""
    from tests.test_gpu_hop_scan import case as scan_case

    c = scan_case("dac-reverse", "5x67")
    N, n_per, n, start = c["N"], c["n_per"], c["n"], c["start"]
    seed, steps, cut = 0, 400, 150  # that file's seed
    grouped = lambda state, first, count, **kw: gpu.hop_evolve_groups(N, c["model"], state, n_per, seed, MASS, c["dt"], first, count, LEFT, RIGHT, reverse=True,
                                                                      trajectory_offset=c["offset"], decoherence=mode, edc_c=EDC_C, **kw)
    zeros = np.zeros((n, 2), dtype=np.int32)
    whole, hops = grouped(start, 0, steps, hops=zeros)
    assert not zeros.any() and hops.min() >= 0 and hops[:, 0].sum() >= 10
    assert same_bits(grouped(start, 0, steps), whole)                                      # hops = null: the same state bits
    first, part = grouped(start, 0, cut, hops=zeros)                                        # two calls, the counters accumulated across them
    second, both = grouped(first, cut, steps - cut, hops=part)
    assert same_bits(second, whole) and np.array_equal(both, hops)
    for g, sl in enumerate(HS.slices(c["n_groups"], n_per)):                                 # the plain call on the slice
        plain = gpu.hop_evolve(N, c["model"], tuple(a[sl] for a in start), seed, MASS, c["dt"][g], 0, steps, LEFT, RIGHT, reverse=True,
                               trajectory_offset=c["offset"] + g * n_per, decoherence=mode, edc_c=EDC_C)
        assert same_bits(plain, tuple(a[sl] for a in whole)), g
    uncorrected = gpu.hop_evolve_groups(N, c["model"], start, n_per, seed, MASS, c["dt"], 0, steps, LEFT, RIGHT, reverse=True, trajectory_offset=c["offset"])
    assert not same_bits(uncorrected, whole)
    done = whole[4] != 0                                                                    # finished trajectories and their counters are frozen
    later, more = grouped(whole, steps, 100, hops=hops)
    assert done.any() and same_bits(tuple(a[done] for a in later), tuple(a[done] for a in whole)) and np.array_equal(more[done], hops[done])


# ---- 3. the phase-space density of a corrected ensemble -------------------------------------------------------------------------------------------
def test_density_of_an_edc_ensemble(gpu):
    """tests/test_gpu_hop_density.py's rule on its 16 x 9 grid: counts and tallies EQUAL, a coherence sum within the count of its cell"""
    ref = reference("dac10-edc")
    c, N = ref["case"], 2
    state = evolve_plain(gpu, c, c["model"], ref["start"], 0, c["steps"], "edc")  # the device's own ensemble: a difference is the binning's alone
    plain = plain_reference("dac10")["end"]
    grid = (LEFT, 0.8, 16, -20.0, 5.0, 9)
    for bin_all in (False, True):
        want = HB.bin(ref["potential"], state, grid, bin_all)
        cells = grid[2] * grid[5]
        counts, coherences, tallies = want[:N * cells].reshape(N, cells), want[N * cells:-2].reshape(N * (N - 1), cells), want[-2:]
        assert (counts.sum(axis=1) > 0).all() and counts.sum(axis=0).max() >= 2 and coherences.any(), "the case tests nothing"
        Cm = HN.states(state[0][HB.cells(state, grid, bin_all)[1] >= 0], ref["potential"])[2]
        last = np.where(Cm[:, 1, :] != 0, Cm[:, 1, :], Cm[:, 0, :])
        assert np.abs(last).min() > 1e-9  # no sign convention can flip between the device and numpy
        got = gpu.hop_bin(N, c["model"], state, grid, bin_all=bin_all)
        assert np.array_equal(got[:N * cells].reshape(N, cells), counts) and np.array_equal(got[-2:], tallies)
        diff = np.abs(got[N * cells:-2].reshape(N * (N - 1), cells) - coherences)
        assert (diff <= counts.sum(axis=0)[None, :]).all()
        rho = gpu.hop_density(N, grid, got, N_TRAJ)
        assert np.array_equal(rho.view(np.float64).view(np.uint64), HB.density(got, N, grid, N_TRAJ).view(np.float64).view(np.uint64))
        if bin_all:  # what the correction is for: the coherence planes of the uncorrected ensemble are larger
            loose = gpu.hop_bin(N, c["model"], plain, grid, bin_all=True)
            damped, free = np.abs(got[N * cells:-2]).sum(), np.abs(loose[N * cells:-2]).sum()
            print(f"hop deco density: sum |coherence sums| {damped / 2 ** 32:.4g} with EDC, {free / 2 ** 32:.4g} without; largest difference {int(diff.max())} unit(s)")
            assert damped < free


# ---- 4. GPLE_ERR_BAD_ARG ------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments(gpu):
    base = plain_reference("dac16")
    lib, ctx = gpu.lib, gpu.ctx
    x, p, b, surface, status = (a.copy() for a in base["start"])
    hops = np.full((N_TRAJ, 2), 7, dtype=np.int32)
    before = tuple(a.copy() for a in (x, p, b, surface, status, hops))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    arrays = dict(x=x.ctypes.data_as(dp), p=p.ctypes.data_as(dp), b=b.ctypes.data_as(dp), surface=surface.ctypes.data_as(ip), status=status.ctypes.data_as(ip))
    nan, inf = float("nan"), float("inf")
    tables = []

    def table(values):
        tables.append(np.ascontiguousarray(values, dtype=np.float64))
        return tables[-1].ctypes.data_as(dp)

    def evolve(**kw):
        a = dict(num_pes=2, model=1, n=N_TRAJ, offset=0, seed=1, mass=MASS, dt=1.0, first=0, steps=3, left=LEFT, right=RIGHT, mode=HD.EDC, edc_c=EDC_C, flags=0,
                 **arrays)
        a.update(kw)
        return lib.gple_hop_evolve_dc(ctx, a["num_pes"], a["model"], a["n"], a["offset"], a["seed"], a["mass"], a["dt"], a["first"], a["steps"], a["left"],
                                      a["right"], a["mode"], a["edc_c"], a["flags"], a["x"], a["p"], a["b"], a["surface"], a["status"])

    def grouped(**kw):
        a = dict(num_pes=2, model=1, groups=1, per=N_TRAJ, offset=0, seed=1, mass=MASS, dt=table([1.0]), first=0, steps=3, left=LEFT, right=RIGHT, mode=HD.EDC,
                 edc_c=EDC_C, flags=0, hops=hops.ctypes.data_as(ip), **arrays)
        a.update(kw)
        return lib.gple_hop_evolve_groups_dc(ctx, a["num_pes"], a["model"], a["groups"], a["per"], a["offset"], a["seed"], a["mass"], a["dt"], a["first"],
                                             a["steps"], a["left"], a["right"], a["mode"], a["edc_c"], a["flags"], a["x"], a["p"], a["b"], a["surface"],
                                             a["status"], a["hops"])

    new = [dict(mode=-1), dict(mode=4), dict(mode=1 << 20), dict(edc_c=-1e-300), dict(edc_c=-1.0), dict(edc_c=nan), dict(edc_c=inf), dict(edc_c=-inf)]
    shared = [dict(num_pes=1), dict(num_pes=4), dict(model=-1), dict(model=3), dict(model=7), dict(model=_capi.PES_USER + 15), dict(mass=0.0), dict(mass=-1.0),
              dict(mass=nan), dict(mass=inf), dict(left=RIGHT), dict(left=7.0), dict(left=nan), dict(right=nan), dict(steps=(1 << 40) + 1),
              dict(offset=(1 << 32) - N_TRAJ + 1)] + [{k: None} for k in arrays]
    for mode in (HD.NONE, HD.EDC, HD.COLLAPSE_HOP, HD.COLLAPSE_ATTEMPT):  # what the old calls refuse is refused in every mode
        for kw in shared + [dict(n=0), dict(dt=0.0), dict(dt=-1.0), dict(dt=nan), dict(dt=inf)]:
            assert evolve(mode=mode, **kw) == BAD_ARG, (mode, kw)
        for kw in shared + [dict(groups=0), dict(per=0), dict(groups=_capi.HOP_MAX_GROUPS + 1, per=1), dict(dt=None), dict(dt=table([0.0])), dict(dt=table([nan]))]:
            assert grouped(mode=mode, **kw) == BAD_ARG, (mode, kw)
    for kw in new:
        assert evolve(**kw) == BAD_ARG and grouped(**kw) == BAD_ARG, kw
    assert same_bits((x, p, b, surface, status, hops), before)  # a refused call writes nothing
    # what is not refused: edc_c = 0; any edc_c in a mode that does not read it; no step at all
    assert evolve(steps=0, edc_c=0.0) == 0 and grouped(steps=0) == 0 and same_bits((x, p, b, surface, status, hops), before)
    for mode in (HD.NONE, HD.COLLAPSE_HOP, HD.COLLAPSE_ATTEMPT):
        assert evolve(mode=mode, edc_c=nan) == 0 and grouped(mode=mode, edc_c=-1.0, hops=None) == 0
    assert evolve(edc_c=0.0) == 0 and not np.array_equal(x, before[0]) and np.array_equal(hops, before[5]) and np.isfinite(b.view(np.float64)).all()


# ---- 5. the drivers -----------------------------------------------------------------------------------------------------------------------------
def test_run_against_the_same_loop_on_the_restatement(gpu, tmp_path):
    kw = dict(model=hopping.DAC, num_pes=2, ln_energy=-2.0, n_traj=512, seed=SEED, dt=2.0, x0=X0, xmin=LEFT, xmax=RIGHT, decoherence="edc", edc_c=EDC_C)
    res = hopping.run(gpu, out_dir=str(tmp_path), **kw)
    narrow = hopping.run(HD.NumpyDecoApi(), **kw)
    wide = hopping.run(HD.NumpyDecoApi(dtype=np.longdouble), **kw)
    assert res["stop"] is not None and res["stop"] == narrow["stop"] == wide["stop"] and len(res["records"]) == len(narrow["records"]) == len(wide["records"]) > 10
    assert hasattr(res["state"][0], "is_cuda") and res["state"][0].is_cuda and res["decoherence"] == "edc" and res["edc_c"] == EDC_C
    worst = {}
    for key in ("x", "p", "E", "populations"):
        got, f64, ld = (np.array([r[key] for r in run["records"]]) for run in (res, narrow, wide))
        worst[key] = np.abs(got - f64).max() / HN.tolerance(np.abs(f64 - ld).max(), f64)
    print("hop deco driver: %d outputs; err / tol %s" % (len(res["records"]), ", ".join(f"{k} {v:.3g}" for k, v in worst.items())))
    for a, b in zip(res["records"], narrow["records"]):
        assert a["t"] == b["t"] and np.array_equal(a["counts"], b["counts"])
    assert all(v <= 1.0 for v in worst.values()), worst
    assert res["scattering_line"] == narrow["scattering_line"]
    plain = hopping.run(gpu, **{**kw, "decoherence": None})
    assert not np.array_equal(plain["records"][-1]["populations"], res["records"][-1]["populations"])
    av = [[float(v) for v in line.split()] for line in open(tmp_path / "averages.txt")]
    assert len(av) == len(res["records"]) and all(len(row) == 8 for row in av)  # the file format is the uncorrected run's


def test_scan_against_the_same_scan_on_the_restatement(gpu):
    kw = dict(model=hopping.DAC, num_pes=2, momenta=[10.0, 16.0, 30.0], n_per_group=128, seed=SEED, dt=[4.0, 2.0, 2.0], chunk_steps=256, x0=X0, xmin=LEFT,
              xmax=RIGHT, decoherence="edc", edc_c=EDC_C)
    res = hopping.scan(gpu, **kw)
    narrow = hopping.scan(HD.NumpyDecoApi(), **kw)
    wide = hopping.scan(HD.NumpyDecoApi(dtype=np.longdouble), **kw)
    assert res["state"][0].is_cuda and res["hop_counts"].is_cuda and res["decoherence"] == "edc"
    assert res["stop"] == narrow["stop"] == wide["stop"] and res["steps"] == narrow["steps"] == wide["steps"] > 0
    assert np.array_equal(res["rows"][:, :6], narrow["rows"][:, :6]) and np.array_equal(narrow["rows"][:, :6], wide["rows"][:, :6])
    assert np.array_equal(res["hop_counts"].cpu().numpy(), narrow["hop_counts"]) and res["hops"].sum() > 0 and res["lines"][0].split()[:6] == narrow["lines"][0].split()[:6]
    worst = {}
    for k, key in enumerate(("c0", "c1", "x", "p", "E")):  # the means per group, under the driver's rule above
        got, f64, ld = (np.asarray(run["rows"], dtype=np.float64)[:, 6 + k] / 128 for run in (res, narrow, wide))
        worst[key] = np.abs(got - f64).max() / HN.tolerance(np.abs(f64 - ld).max(), f64)
    print(f"hop deco scan driver: {res['steps']} steps, hops {res['hops']}; err / tol " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst
