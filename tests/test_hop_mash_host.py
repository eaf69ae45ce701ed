"""CPU: the numpy restatement of the MASH trajectories (tests/hop_mash_numpy.py), which the GPU tests lean on, the drivers hopping.run and
hopping.scan with method="mash" on the numpy stand-in api, and the new symbols of the built library (the test here that fails without the
feature).  Every bound is reasoned where it stands; none comes from what the restatement gives."""
import re
from pathlib import Path

import numpy as np
import pytest

import gaussian_process_liouville_equation_amd as pkg
from gaussian_process_liouville_equation_amd import _capi, hopping
from tests import hop_mash_numpy as HA
from tests import hop_mf_numpy as HM
from tests import hop_numpy as HN
from tests import hop_scan_numpy as HS

EPS = np.finfo(np.float64).eps
MASS, X0, LEFT, RIGHT = 2000.0, -4.0, -6.0, 6.0
FAR = 1e3
NAMES = ("hop_sample_mash", "hop_sample_groups_mash", "hop_evolve_mash", "hop_evolve_groups_mash")


def packet(p0):
    return X0, p0, 1.0 / (2.0 * p0 / 20.0), p0 / 20.0


def ensemble(potential, n, p0, seed=0, surface0=0, dtype=np.float64):
    return HA.sample(potential, 2, n, seed, *packet(p0), surface0, dtype=dtype)


def widen(state):
    x, p, b, surface, status = state
    return x.astype(np.longdouble), p.astype(np.longdouble), b.astype(np.clongdouble), surface, status


def same_bits(a, b):
    return all(np.array_equal(u, v) and u.dtype == v.dtype for u, v in zip(a, b))


def test_the_library_exports_and_the_binding_declares_the_four_entry_points():
    lib = pkg.load_library()  # no HIP call at load time: works without a GPU
    text = (Path(__file__).resolve().parent.parent / "include" / "gple.h").read_text()
    for name in NAMES:
        assert name in _capi.GPLE_SYMBOLS
        f = getattr(lib, "gple_" + name)
        assert f.argtypes is not None and len(f.argtypes) == len(_capi.SIGNATURES[name][1])
        assert hasattr(_capi.Api, name)
        assert re.search(r"\bint\s+gple_%s\s*\(" % name, text)
    assert re.search(r"GPLE_TIMER_HOP_MASH\s*=\s*17\b", text) and _capi.TIMER_HOP_MASH == 17
    assert hopping.MASH == "mash" and hopping.METHODS == ("fssh", "ehrenfest")


# ---- the sample ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("surface0", [0, 1])
def test_the_sample_draws_the_spin_with_the_density_2s_on_the_side_of_the_start_surface(surface0):
    n, seed = 65536, 5
    pot = HN.builtin(HN.DAC, 2)
    s, w1 = HA.spin(np.arange(n), seed)
    assert (s > 0).all() and (s <= 1).all() and (w1 >= 0).all() and (w1 < 1).all()
    x, p, b, surface, status = HA.sample(pot, 2, n, seed, *packet(16.0), surface0)
    plain = HN.sample(pot, 2, n, seed, *packet(16.0), surface0)
    assert same_bits((x, p, surface, status), (plain[0], plain[1], plain[3], plain[4]))  # the bits of the fewest-switches sample
    assert (surface == surface0).all() and (status == 0).all() and surface.dtype == status.dtype == np.int32
    _, _, C, _ = HN.states(x, pot)
    w = HA.norms(HA.adiabatic(C, b))
    # density 2 s on (0, 1]: E s = 2/3, E s^2 = 1/2, E s^4 = 1/3, so Var s = 1/18, Var s^2 = 1/12, and |c_a|^2 = (1 + s) / 2 has the mean 5/6
    # and the variance 1/72; each mean of n draws within 6 standard errors
    for got, mean, var in ((s.mean(), 2.0 / 3.0, 1.0 / 18.0), ((s * s).mean(), 0.5, 1.0 / 12.0), (w[:, surface0].mean(), 5.0 / 6.0, 1.0 / 72.0)):
        assert abs(got - mean) <= 6.0 * np.sqrt(var / n), (got, mean)
    assert np.abs(HA.norms(b).sum(axis=1) - 1.0).max() <= 4 * EPS
    assert np.array_equal(HA.side(HA.adiabatic(C, b)), np.full(n, surface0))
    assert np.abs(w[:, surface0] - (1.0 + s) / 2.0).max() <= 8 * EPS  # what was drawn is what the adiabatic populations show
    part = HA.sample(pot, 2, 100, seed, *packet(16.0), surface0, trajectory_offset=300)  # a slice with its offset
    assert same_bits(part, tuple(a[300:400] for a in (x, p, b, surface, status)))
    other = HA.sample(pot, 2, 400, seed + 1, *packet(16.0), surface0)
    assert not np.array_equal(other[2], b[:400])
    with pytest.raises(ValueError):
        HA.sample(HN.builtin(HN.TSAC, 3), 3, 8, seed, *packet(16.0), 0)


def test_the_grouped_sample_is_the_plain_one_per_group_and_keeps_the_zero_sigma_select():
    pot = HN.builtin(HN.DAC, 2)
    packets = np.array([packet(10.0), packet(16.0), (X0, 24.0, 0.0, 0.0)])
    got = HA.sample_groups(pot, 2, 50, 9, packets, 1, trajectory_offset=7)
    for g, sl in enumerate(HS.slices(3, 50)):
        if packets[g, 2] > 0:
            assert same_bits(HA.sample(pot, 2, 50, 9, *packets[g], 1, trajectory_offset=7 + 50 * g), tuple(a[sl] for a in got)), g
    assert (got[0][100:] == X0).all() and (got[1][100:] == 24.0).all() and len(np.unique(got[2][100:, 0])) == 50  # a point, the spins still drawn
    plain = HS.sample_groups(pot, 2, 50, 9, packets, 1, trajectory_offset=7)
    assert same_bits((got[0], got[1], got[3], got[4]), (plain[0], plain[1], plain[3], plain[4]))


# ---- the step -----------------------------------------------------------------------------------------------------------------------------------------
def test_the_step_is_unitary():
    pot = HN.builtin(HN.DAC, 2)
    _, diag = HA.evolve(pot, ensemble(pot, 64, 16.0), MASS, 1.0, 1000, -FAR, FAR, history=True)
    assert len(diag["steps"]) == 1000 and diag["hops"].sum() > 0
    assert max(np.abs(st["norm"] - 1.0).max() for st in diag["steps"]) <= 1e-12


def test_a_taken_hop_conserves_the_energy_and_the_integrator_is_of_second_order():
    pot = HN.builtin(HN.DAC, 2)
    start = ensemble(pot, 64, 16.0, seed=3)
    _, E, _, _ = HN.states(start[0], pot)
    e0 = start[1] ** 2 / 2.0 / MASS + E[:, 0]

    def deviation(dt, steps):
        """the largest |p^2 / 2m + E_a - its value at the start| over the steps, per trajectory, and who had no event"""
        _, diag = HA.evolve(pot, start, MASS, dt, steps, -FAR, FAR, history=True)
        dev = np.zeros(64)
        for st in diag["steps"]:
            assert len(st["index"]) == 64
            dev = np.maximum(dev, np.abs(st["E_after"] - e0))
            # p' = sgn(p) sqrt(p^2 + 2m (E_a - E_k)): r, the root, its square, the division by 2m and the two sums are a handful of roundings of
            # terms no larger than the kinetic energy and the two adiabatic energies
            scale = st["p_before"] ** 2 / 2.0 / MASS + np.abs(st["E_before"]) + np.abs(st["E_after"])
            assert (np.abs(st["E_after"] - st["E_before"])[st["taken"]] <= 8 * EPS * scale[st["taken"]]).all()
            assert np.array_equal(st["E_after"][~(st["taken"] | st["stuck"])], st["E_before"][~(st["taken"] | st["stuck"])])
        return dev, (diag["hops"] + diag["frustrated"]) == 0, diag["hops"].sum()

    coarse, quiet_coarse, hops = deviation(2.0, 500)
    fine, quiet_fine, _ = deviation(1.0, 1000)
    quiet = quiet_coarse & quiet_fine
    assert hops >= 10 and quiet.sum() >= 20, "the case tests nothing"
    assert abs(coarse[quiet].max() / fine[quiet].max() - 4.0) <= 0.1


def test_the_surface_is_the_side_for_every_trajectory_that_was_never_frustrated():
    pot = HN.builtin(HN.DAC, 2)
    for p0, dt, steps in ((10.0, 2.0, 900), (16.0, 1.0, 500)):
        _, diag = HA.evolve(pot, ensemble(pot, 128, p0), MASS, dt, steps, LEFT, RIGHT, history=True)
        clean = diag["frustrated"] == 0
        assert clean.sum() >= 50 and diag["hops"][clean].sum() >= 10
        for st in diag["steps"]:
            keep = clean[st["index"]]
            assert np.array_equal(st["a"][keep], st["side"][keep])


def test_a_frustrated_hop_reflects_once():
    """DAC at p0 = 10: at the frustrated step p is exactly negated and the surface stays; while the side stays away from the surface nothing
    happens again; the crossing back changes nothing"""
    pot = HN.builtin(HN.DAC, 2)
    n = 293
    _, diag = HA.evolve(pot, ensemble(pot, n, 10.0), MASS, 2.0, 900, LEFT, RIGHT, history=True)
    assert diag["frustrated"].sum() >= 10, "the case tests nothing"
    away = np.zeros(n, dtype=bool)  # frustrated, and the side has not come back to the surface since
    came_back = 0
    for st in diag["steps"]:
        i, stuck, taken = st["index"], st["stuck"], st["taken"]
        assert np.array_equal(st["p"][stuck], -st["p_before"][stuck]) and np.array_equal(st["a"][stuck], st["a_before"][stuck])
        assert (st["side"][stuck] != st["a"][stuck]).all() and (st["side_old"][stuck] == st["a"][stuck]).all()
        was = away[i]
        persists = was & (st["side"] != st["a_before"])
        assert not (stuck | taken)[persists].any() and np.array_equal(st["p"][persists], st["p_before"][persists])
        back = was & (st["side"] == st["a_before"])  # the crossing back
        assert not (stuck | taken)[back].any() and np.array_equal(st["p"][back], st["p_before"][back]) and np.array_equal(st["a"][back], st["a_before"][back])
        came_back += int(back.sum())
        away[i] = (was & ~back) | stuck
    assert came_back >= 5, "no reflected trajectory crossed back: the case tests nothing"


@pytest.mark.parametrize("model,p0,dt,steps,surface0", [(HN.DAC, 10.0, 2.0, 900, 0), (HN.SAC, 10.0, 2.0, 400, 0), (HN.ECR, 10.0, 4.0, 700, 1)])
def test_the_sign_of_the_eigenvectors_changes_nothing(model, p0, dt, steps, surface0):
    pot = HN.builtin(model, 2)
    start = ensemble(pot, 96, p0, surface0=surface0)
    plain, d0 = HA.evolve(pot, start, MASS, dt, steps, LEFT, RIGHT)
    flipped, d1 = HA.evolve(pot, start, MASS, dt, steps, LEFT, RIGHT, flip=True)
    wide, _ = HA.evolve(pot, widen(start), MASS, dt, steps, LEFT, RIGHT)
    assert d0["hops"].sum() >= 5 and not HA.set_aside(d0).any()
    assert np.array_equal(plain[3], flipped[3]) and np.array_equal(plain[4], flipped[4])
    assert np.array_equal(d0["hops"], d1["hops"]) and np.array_equal(d0["frustrated"], d1["frustrated"])
    for q in range(3):  # the rounding floor: the distance of float64 to long double
        assert np.abs(plain[q] - flipped[q]).max() <= HN.tolerance(np.abs(plain[q] - wide[q]).max(), plain[q])


@pytest.mark.parametrize("surface0", [0, 1])
def test_no_events_where_there_is_no_coupling(surface0):
    """a tabulated model whose coupling entry is exactly zero and whose levels never cross: 0 and a well 0.11 - 0.10 exp(-0.28 x^2) above it"""
    nodes = -8.0 + np.arange(257) / 16.0
    V, dV = np.zeros((257, 2, 2)), np.zeros((257, 2, 2))
    V[:, 1, 1], dV[:, 1, 1] = 0.11 - 0.10 * np.exp(-0.28 * nodes * nodes), 2 * 0.10 * 0.28 * nodes * np.exp(-0.28 * nodes * nodes)
    pot = HN.table(HN.FunctionTable(-8.0, 1.0 / 16.0, V, dV))
    start = ensemble(pot, 96, 16.0, surface0=surface0)
    end, diag = HA.evolve(pot, start, MASS, 1.0, 1500, LEFT, RIGHT, history=True)
    assert not diag["hops"].any() and not diag["frustrated"].any() and (end[3] == surface0).all() and (end[4] != 0).sum() >= 48
    assert all((st["a"] == surface0).all() and (st["side"] == surface0).all() for st in diag["steps"])
    assert np.abs(np.abs(end[2]) - np.abs(start[2])).max() <= 1e-12  # the amplitudes only turn


def test_evolve_carries_nothing_hidden_and_a_slice_or_a_group_is_the_plain_call():
    pot = HN.builtin(HN.DAC, 2)
    start = ensemble(pot, 64, 10.0)
    whole, diag = HA.evolve(pot, start, MASS, 2.0, 400, LEFT, RIGHT)
    assert diag["frustrated"].sum() >= 3 and diag["hops"].sum() >= 10 and (whole[4] != 0).any()
    state = start
    for _ in range(400):  # 400 calls of one step: the cuts fall between a reflection and the crossing back too
        state, _ = HA.evolve(pot, state, MASS, 2.0, 1, LEFT, RIGHT)
    assert same_bits(state, whole)
    assert same_bits(HA.evolve(pot, tuple(a[20:] for a in start), MASS, 2.0, 400, LEFT, RIGHT)[0], tuple(a[20:] for a in whole))
    later, _ = HA.evolve(pot, whole, MASS, 2.0, 200, LEFT, RIGHT)  # a finished trajectory is frozen
    done = whole[4] != 0
    assert same_bits(tuple(a[done] for a in later), tuple(a[done] for a in whole))
    dt = np.array([2.0, 1.0, 2.0, 0.5])
    grouped, hops, _ = HA.evolve_groups(pot, start, 16, MASS, dt, 300, LEFT, RIGHT, hops=np.ones((64, 2), dtype=np.int32))
    for g, sl in enumerate(HS.slices(4, 16)):
        alone, d = HA.evolve(pot, tuple(a[sl] for a in start), MASS, dt[g], 300, LEFT, RIGHT)
        assert same_bits(alone, tuple(a[sl] for a in grouped)), g
        assert np.array_equal(hops[sl, 0], 1 + d["hops"]) and np.array_equal(hops[sl, 1], 1 + d["frustrated"])


def test_the_five_gpu_cases_set_no_trajectory_aside():
    """what tests/test_gpu_hop_mash.py may set aside, counted on the restatement alone, with that file's cases and its seed"""
    from tests import hop_mash_cases as G

    assert G.SEED == 0 and G.N_TRAJ == 293 and len(G.CASES) == 5
    for name in G.CASES:
        ref = G.reference(name)
        assert not HA.set_aside(ref["diag"]).any(), name
        assert ref["diag"]["hops"].sum() >= 10, name
    assert G.reference("dac10")["diag"]["frustrated"].sum() >= 10


# ---- the drivers --------------------------------------------------------------------------------------------------------------------------------------
def parse(path):
    return [[float(v) for v in line.split()] for line in open(path)]


RUN = dict(model=hopping.DAC, num_pes=2, ln_energy=-2.0, n_traj=48, seed=4, dt=4.0, x0=X0, xmin=LEFT, xmax=RIGHT)


def test_run_until_nobody_runs(tmp_path):
    api = HA.NumpyMashApi()
    res = hopping.run(api, out_dir=str(tmp_path), method="mash", **RUN)
    assert res["method"] == "mash" and res["stop"] is not None and "NO TRAJECTORY IS RUNNING" in res["stop"]
    step, count = res["output_step"], len(res["records"])
    # one sample, then an observe per output time and an evolve of output_step steps between two of them
    assert api.calls == [("sample_mash", 48)] + [c for _ in range(count - 1) for c in (("observe",), ("evolve_mash", step))] + [("observe",)]
    t, av = parse(tmp_path / "t.txt"), parse(tmp_path / "averages.txt")
    assert len(t) == len(av) == count and sorted(p.name for p in tmp_path.iterdir()) == ["averages.txt", "t.txt"]
    for rec, (tt,), line in zip(res["records"], t, av):
        want = [rec["t"], rec["E"], rec["x"], rec["p"], *(rec["counts"].sum(axis=0) / 48), *rec["populations"]]
        assert np.allclose([tt] + line, [rec["t"]] + want, rtol=1e-5, atol=1e-300)
    last = res["records"][-1]
    assert last["counts"][0].sum() == 0 and last["counts"].sum() == 48
    line = [float(v) for v in res["scattering_line"].split()]
    assert len(line) == 6 and line[5] == 0.0 and abs(sum(line[1:5]) - 1.0) < 1e-5 and abs(line[0] + 2.0) < 1e-5
    assert np.array_equal(res["scattered"], last["counts"][1:] / 48)
    # the same loop by hand on the restatement
    pot, s = HN.builtin(HN.DAC, 2), res["setup"]
    state = HA.sample(pot, 2, 48, 4, s["x0"], s["p0"], s["sigma_x"], s["sigma_p"], 0)
    for _ in range(count - 1):
        state, _ = HA.evolve(pot, state, MASS, 4.0, step, LEFT, RIGHT)
    assert same_bits(state, res["state"])


def test_run_until_the_total_time_and_what_it_refuses(tmp_path):
    p0 = float(np.sqrt(2.0 * MASS * np.exp(-2.0)))
    kw = dict(RUN, model=hopping.SAC, dt=8.0, sigma_p=p0 / 2.0)  # a packet as wide as its momentum: some trajectories crawl
    res = hopping.run(HA.NumpyMashApi(), out_dir=str(tmp_path), method="mash", **kw)
    assert res["stop"] is None and res["steps"] + res["output_step"] > res["total_step"] >= res["steps"]
    last = res["records"][-1]
    line = [float(v) for v in res["scattering_line"].split()]
    assert last["counts"][0].sum() > 0 and abs(line[5] - last["counts"][0].sum() / 48) < 1e-5 and abs(line[0] - p0) < 1e-4  # not DAC: p0
    early = hopping.run(HA.NumpyMashApi(), method="mash", max_outputs=1, **RUN)
    assert len(early["records"]) == 1 and [float(v) for v in early["scattering_line"].split()][1:] == [0.0, 0.0, 0.0, 0.0, 1.0]
    bad = [dict(decoherence="edc"), dict(decoherence="collapse_hop"), dict(reverse_frustrated=True), dict(phase_grid=(8, 8)), dict(window="triangle"),
           dict(gamma=0.3), dict(num_pes=3, model=hopping.TSAC), dict(method="mesh")]
    for kw in bad:
        api = HA.NumpyMashApi()
        with pytest.raises(ValueError):
            hopping.run(api, **{"method": "mash", **RUN, **kw})
        assert api.calls == [], kw  # refused before anything ran


SCAN = dict(model=hopping.DAC, num_pes=2, momenta=[10.0, 16.0, 30.0], n_per_group=12, seed=1, dt=[2.0, 2.0, 1.0], x0=X0, xmin=LEFT, xmax=RIGHT)


@pytest.mark.parametrize("fixed", [True, False])
def test_scan_until_nobody_runs(tmp_path, fixed):
    api = HA.NumpyMashApi()
    res = hopping.scan(api, fixed=fixed, chunk_steps=128, out_dir=str(tmp_path), method="mash", **SCAN)
    assert res["method"] == "mash" and res["stop"] is not None and "NO TRAJECTORY IS RUNNING" in res["stop"] and res["steps"] % 128 == 0
    chunks = res["steps"] // 128
    assert api.calls == [("sample_groups_mash", 3, 12), ("observe_groups",)] + [("evolve_groups_mash", 128), ("observe_groups",)] * chunks
    pot = HN.builtin(HN.DAC, 2)
    packets = [[s["x0"], s["p0"], 0.0 if fixed else s["sigma_x"], 0.0 if fixed else s["sigma_p"]] for s in res["setups"]]
    start = HA.sample_groups(pot, 2, 12, 1, packets, 0)
    total = np.zeros((3, 2))
    for g, sl in enumerate(HS.slices(3, 12)):  # every group is the plain call on its slice
        end, diag = HA.evolve(pot, tuple(a[sl] for a in start), MASS, SCAN["dt"][g], res["steps"], LEFT, RIGHT)
        assert np.array_equal(res["rows"][g], HN.observe(pot, end, MASS))
        total[g] = diag["hops"].sum(), diag["frustrated"].sum()
    assert res["rows"].shape == (3, 11) and res["hop_counts"].shape == (36, 2) and res["hop_counts"].dtype == np.int32
    assert np.array_equal(res["hops"], total[:, 0] / 12) and np.array_equal(res["frustrated"], total[:, 1] / 12) and total[:, 0].sum() > 0
    if fixed:  # the packet is a point, the spins are still drawn: the trajectories of a group differ
        assert all(len(np.unique(res["state"][0][sl])) > 1 for sl in HS.slices(3, 12))
    lines = parse(tmp_path / "scan.txt")  # head, 4 channels, running, their 5 standard errors, hops, frustrated, drift
    assert len(lines) == 3 and all(len(line) == 1 + 5 + 5 + 3 for line in lines) and sorted(p.name for p in tmp_path.iterdir()) == ["scan.txt"]
    for g, line in enumerate(lines):
        f = np.concatenate([res["scattered"][g].reshape(-1), [0.0]])
        want = [np.log(res["setups"][g]["p0"] ** 2 / 2.0 / MASS), *f, *np.sqrt(f * (1.0 - f) / 12), total[g, 0] / 12, total[g, 1] / 12, res["energy_drift"][g]]
        assert np.allclose(line, want, rtol=1e-5, atol=1e-300) and abs(f.sum() - 1.0) < 1e-12


def test_scan_stops_at_max_steps_and_what_it_refuses():
    res = hopping.scan(HA.NumpyMashApi(), fixed=False, chunk_steps=64, max_steps=200, method="mash", **SCAN)
    assert res["stop"] is None and res["steps"] == 200 and res["running"].sum() > 0
    api = HA.NumpyMashApi()
    other = hopping.scan(api, fixed=False, chunk_steps=77, max_steps=200, method="mash", **SCAN)
    assert [c for c in api.calls if c[0] == "evolve_groups_mash"] == [("evolve_groups_mash", 77), ("evolve_groups_mash", 77), ("evolve_groups_mash", 46)]
    assert same_bits(res["state"], other["state"]) and res["lines"] == other["lines"] and np.array_equal(res["hop_counts"], other["hop_counts"])
    for bad in (dict(decoherence="edc"), dict(reverse_frustrated=True), dict(window="square"), dict(gamma=0.2), dict(num_pes=3, model=hopping.TSAC),
                dict(method="mesh")):
        api = HA.NumpyMashApi()
        with pytest.raises(ValueError):
            hopping.scan(api, **{"method": "mash", **SCAN, **bad})
        assert api.calls == [], bad


def test_the_other_methods_make_the_calls_they_made():
    """method="fssh" and "ehrenfest": on the stand-in that also has the four new methods "fssh" records exactly the calls of the parent commit,
    and on stand-ins that know nothing of the new methods both still run"""
    for api in (HA.NumpyMashApi(), HN.NumpyHopApi()):
        res = hopping.run(api, **RUN)
        count, step = len(res["records"]), res["output_step"]
        assert api.calls == [("sample", 48)] + [c for k in range(count - 1) for c in (("observe",), ("evolve", k * step, step))] + [("observe",)]
    api = HM.NumpyMfApi()
    res = hopping.run(api, method="ehrenfest", **RUN)
    count = len(res["records"])
    assert not any(hasattr(api, name) for name in NAMES)
    assert api.calls == [("sample", 48)] + [c for _ in range(count - 1) for c in (("observe_mf",), ("evolve_mf", step))] + [("observe_mf",)]
    for api in (HA.NumpyMashApi(), HS.NumpyScanApi()):
        hopping.scan(api, fixed=False, chunk_steps=128, max_steps=256, **dict(SCAN, n_per_group=4))
        assert api.calls == [("sample_groups", 3, 4), ("observe_groups",), ("evolve_groups", 0, 128), ("observe_groups",), ("evolve_groups", 128, 128),
                             ("observe_groups",)]
    api = HM.NumpyMfApi()
    hopping.scan(api, fixed=False, chunk_steps=128, max_steps=256, method="ehrenfest", **dict(SCAN, n_per_group=4))
    assert api.calls == [("sample_groups", 3, 4), ("observe_groups_mf",), ("evolve_groups_mf", 128), ("observe_groups_mf",), ("evolve_groups_mf", 128),
                         ("observe_groups_mf",)]
