"""CPU: the numpy restatement of the Ehrenfest (mean-field) step (tests/hop_mf_numpy.py), which the GPU tests lean on, hopping.unpack_mf, the
drivers hopping.run and hopping.scan with method="ehrenfest" on the numpy stand-in api, and the new symbols of the built library (the one test
here that fails without the feature)."""
import re
from pathlib import Path

import numpy as np
import pytest

import gaussian_process_liouville_equation_amd as pkg
from gaussian_process_liouville_equation_amd import _capi, exact, hopping
from tests import hop_mf_numpy as HM
from tests import hop_numpy as HN
from tests import hop_scan_numpy as HS

MASS, X0, LEFT, RIGHT = 2000.0, -4.0, -6.0, 6.0
FAR = 1e3


def ensemble(potential, num_pes, n, p0, seed=11, surface0=0, dtype=np.float64):
    return HN.sample(potential, num_pes, n, seed, X0, p0, 1.0 / (2.0 * p0 / 20.0), p0 / 20.0, surface0=surface0, dtype=dtype)


def same_bits(a, b):
    return all(np.array_equal(u, v) and u.dtype == v.dtype for u, v in zip(a, b))


def test_the_library_exports_and_the_binding_declares_the_mean_field_entry_points():
    lib = pkg.load_library()  # no HIP call at load time: works without a GPU
    text = (Path(__file__).resolve().parent.parent / "include" / "gple.h").read_text()
    for name in ("hop_evolve_mf", "hop_evolve_groups_mf", "hop_observe_mf", "hop_observe_groups_mf"):
        assert name in _capi.GPLE_SYMBOLS
        f = getattr(lib, "gple_" + name)
        assert f.argtypes is not None and len(f.argtypes) == len(_capi.SIGNATURES[name][1])
        assert hasattr(_capi.Api, name)
        assert re.search(r"\bint\s+gple_%s\s*\(" % name, text)
    assert re.search(r"GPLE_TIMER_HOP_MF\s*=\s*15\b", text) and _capi.TIMER_HOP_MF == 15
    assert callable(hopping.unpack_mf) and hopping.METHODS == ("fssh", "ehrenfest")


def test_the_amplitudes_stay_normalised():
    pot = HN.builtin(HN.DAC, 2)
    (x, p, b, surface, status), _ = HM.evolve(pot, ensemble(pot, 2, 64, 16.0), MASS, 1.0, 1000, -FAR, FAR)
    assert (status == 0).all() and (np.abs(b) ** 2).min(axis=0).max() > 1e-3  # both levels are populated: the step mixed them
    worst = np.abs(np.sum(HM.norms(b), axis=1) - 1.0).max()
    print(f"mean field: | |b|^2 - 1 | after 1000 steps {worst:.3g}")
    assert worst <= 1e-12


def test_the_integrator_is_of_second_order():
    """The step is time-symmetric: the largest deviation of p^2 / 2m + b^dagger V b from its start value over the steps up to t = 1000, over 64
    trajectories on DAC (smooth) at p0 = 16 through both crossings, falls by a factor of 4 per halving of dt"""
    pot = HN.builtin(HN.DAC, 2)
    state = ensemble(pot, 2, 64, 16.0)
    worst = [HM.evolve(pot, state, MASS, dt, int(1000 / dt), -FAR, FAR)[1]["drift"].max() for dt in (2.0, 1.0, 0.5)]
    ratios = [worst[0] / worst[1], worst[1] / worst[2]]
    print("mean field: energy deviation %.3g %.3g %.3g, ratios %.4f %.4f" % (*worst, *ratios))
    assert all(3.9 <= r <= 4.1 for r in ratios), ratios


@pytest.mark.parametrize("model,N", [(HN.DAC, 2), (HN.SAC, 2), (HN.TSAC, 3)])
def test_the_diabatic_force_is_the_adiabatic_quadratic_form(model, N):
    """b^dagger Fd b = c^dagger (C^T Fd C) c with c = C^T b.  Relative to what: sum_ij |Fd_ij| bounds |f| for a unit b, and every rounding
    error of either form is a multiple of eps times terms bounded by it"""
    pot = HN.builtin(model, N)
    rng = np.random.default_rng(5)
    x = np.linspace(-5.0, 5.0, 200)  # not x = 0, where the force matrix of DAC vanishes
    b = rng.normal(size=(200, N)) + 1j * rng.normal(size=(200, N))
    b /= np.sqrt(np.sum(np.abs(b) ** 2, axis=1))[:, None]
    _, Fd = pot(x)
    _, _, C, F = HN.states(x, pot)
    c = np.einsum("mik,mi->mk", C, b)
    want = np.einsum("mk,mkl,ml->m", np.conj(c), F, c).real
    scale = np.abs(Fd).sum(axis=(1, 2))
    worst = (np.abs(HM.force(Fd, b) - want) / scale).max()
    print(f"mean field force {model}: relative difference {worst:.3g}")
    assert worst <= 1e-14


@pytest.mark.parametrize("model,N,p0,dt,steps", [(HN.DAC, 2, 10.0, 2.0, 600), (HN.TSAC, 3, 10.0, 4.0, 300)])
def test_the_sign_of_the_eigenvectors_changes_nothing(model, N, p0, dt, steps):
    """W enters as W_rk W_qk only, and (-a)(-b) = a b exactly: not a bit moves"""
    pot = HN.builtin(model, N)
    state = ensemble(pot, N, 96, p0)
    plain, _ = HM.evolve(pot, state, MASS, dt, steps, LEFT, RIGHT)
    flipped, _ = HM.evolve(pot, state, MASS, dt, steps, LEFT, RIGHT, flip=True)
    assert same_bits(plain, flipped) and (plain[4] != 0).any()


def test_evolve_carries_nothing_hidden_and_a_slice_is_a_slice():
    pot = HN.builtin(HN.DAC, 2)
    state = ensemble(pot, 2, 48, 10.0)
    whole, _ = HM.evolve(pot, state, MASS, 2.0, 900, LEFT, RIGHT)
    half, _ = HM.evolve(pot, state, MASS, 2.0, 350, LEFT, RIGHT)
    rest, _ = HM.evolve(pot, half, MASS, 2.0, 550, LEFT, RIGHT)
    assert same_bits(whole, rest) and (whole[4] != 0).any() and (whole[4] == 0).any()
    part, _ = HM.evolve(pot, tuple(a[20:] for a in state), MASS, 2.0, 900, LEFT, RIGHT)
    assert same_bits(tuple(a[20:] for a in whole), part)
    assert whole[3] is state[3]  # the surface is handed through
    later, _ = HM.evolve(pot, whole, MASS, 2.0, 100, LEFT, RIGHT)  # a finished trajectory is frozen
    done = whole[4] != 0
    assert same_bits(tuple(a[done] for a in later), tuple(a[done] for a in whole))
    # groups: a slice per group with its own time step; one time step for all is the plain call
    dt = np.array([2.0, 1.0, 4.0])
    grouped, _ = HM.evolve_groups(pot, state, 16, MASS, dt, 300, LEFT, RIGHT)
    for g, sl in enumerate(HS.slices(3, 16)):
        assert same_bits(tuple(a[sl] for a in grouped), HM.evolve(pot, tuple(a[sl] for a in state), MASS, dt[g], 300, LEFT, RIGHT)[0])
    assert same_bits(HM.evolve_groups(pot, state, 16, MASS, np.full(3, 2.0), 900, LEFT, RIGHT)[0], whole)
    rows = HM.observe_groups(pot, grouped, 16, MASS)
    assert rows.shape == (3, 12) and np.array_equal(rows[1], HM.observe(pot, tuple(a[16:32] for a in grouped), MASS))


def test_unpack_mf_and_the_three_level_layout():
    pot = HN.builtin(HN.TSAC, 3)
    state, _ = HM.evolve(pot, ensemble(pot, 3, 40, 10.0), MASS, 4.0, 600, LEFT, RIGHT)
    sums = HM.observe(pot, state, MASS)
    rec = hopping.unpack_mf(sums, 3, 40)
    _, E, C, _ = HN.states(state[0], pot)
    w = np.abs(np.einsum("mik,mi->mk", C, state[2])) ** 2
    assert rec["weights"].shape == (3, 3) and rec["n_status"].shape == (3,) and rec["counts"] is rec["weights"]
    for status in range(3):
        assert rec["n_status"][status] == np.sum(state[4] == status)
        assert np.abs(rec["weights"][status] - w[state[4] == status].sum(axis=0)).max() < 1e-12
        assert abs(rec["weights"][status].sum() - rec["n_status"][status]) < 1e-11  # a trajectory's weights add up to one
    assert min(rec["n_status"][0], rec["n_status"][2]) >= 5 and rec["n_status"].sum() == 40
    assert abs(rec["populations"].sum() - 1.0) < 1e-12 and abs(rec["x"] - state[0].mean()) < 1e-12 and abs(rec["p"] - state[1].mean()) < 1e-12
    assert abs(rec["E"] - np.mean(state[1] ** 2 / 2.0 / MASS + np.sum(w * E, axis=1))) < 1e-12
    with pytest.raises(ValueError):
        hopping.unpack_mf(np.zeros(15), 2, 40)
    odd = (state[0], state[1], state[2], state[3], np.where(np.arange(40) < 3, 7, state[4]).astype(np.int32))  # a status out of range: no weight, no count
    skipped = hopping.unpack_mf(HM.observe(pot, odd, MASS), 3, 40)
    assert skipped["n_status"].sum() == 37 and abs(skipped["weights"].sum() - 37.0) < 1e-11 and skipped["x"] == rec["x"]


def parse(path):
    return [[float(v) for v in line.split()] for line in open(path)]


def check_files(res, out_dir, num_pes):
    t, av = parse(out_dir / "t.txt"), parse(out_dir / "averages.txt")
    assert len(t) == len(av) == len(res["records"])
    for rec, (tt,), line in zip(res["records"], t, av):
        assert len(line) == 4 + num_pes  # t <E> <x> <p> and the mean |c_k|^2: no active-surface columns
        assert np.allclose([tt] + line, [rec["t"], rec["t"], rec["E"], rec["x"], rec["p"], *rec["populations"]], rtol=1e-5, atol=1e-300)


RUN = dict(model=hopping.DAC, num_pes=2, ln_energy=-2.0, n_traj=48, seed=4, dt=4.0, x0=X0, xmin=LEFT, xmax=RIGHT)


def test_run_until_nobody_runs(tmp_path):
    api = HM.NumpyMfApi()
    res = hopping.run(api, out_dir=str(tmp_path), method="ehrenfest", **RUN)
    assert res["method"] == "ehrenfest" and res["stop"] is not None and "NO TRAJECTORY IS RUNNING" in res["stop"]
    step = res["output_step"]
    assert step == int(res["setup"]["output_time"] / 4.0) and res["steps"] <= res["total_step"]
    # one sample, then an observe_mf per output time and an evolve_mf of output_step steps between two of them
    calls = api.calls
    assert calls[0] == ("sample", 48) and calls[1] == ("observe_mf",) and len(calls) == 2 * len(res["records"])
    assert calls[2::2] == [("evolve_mf", step)] * (len(res["records"]) - 1) and all(c == ("observe_mf",) for c in calls[3::2])
    check_files(res, tmp_path, 2)
    last = res["records"][-1]
    assert last["n_status"][hopping.RUNNING] == 0 and last["n_status"].sum() == 48 and abs(last["weights"].sum() - 48.0) < 1e-10
    line = [float(v) for v in res["scattering_line"].split()]
    assert len(line) == 1 + 2 * 2 + 1 and line[-1] == 0.0 and abs(sum(line[1:]) - 1.0) < 1e-5 and abs(line[0] + 2.0) < 1e-5
    assert np.array_equal(res["scattered"], last["weights"][1:] / 48)
    assert 0.0 < res["scattered"][1, 1] < 1.0  # a transmitted trajectory carries weight on both surfaces: no active surface to count
    assert res["state"][3] is not None and (np.asarray(res["state"][3]) == 0).all()  # the surface of the sample, untouched


def test_run_until_the_total_time_and_what_it_refuses(tmp_path):
    p0 = float(np.sqrt(2.0 * MASS * np.exp(-2.0)))
    kw = dict(RUN, model=hopping.SAC, dt=8.0, sigma_p=p0 / 2.0)  # a packet as wide as its momentum: some trajectories crawl
    res = hopping.run(HM.NumpyMfApi(), out_dir=str(tmp_path), method="ehrenfest", **kw)
    assert res["stop"] is None and res["steps"] + res["output_step"] > res["total_step"] >= res["steps"]
    last = res["records"][-1]
    assert last["n_status"][hopping.RUNNING] > 0 and last["n_status"].sum() == 48
    check_files(res, tmp_path, 2)
    line = [float(v) for v in res["scattering_line"].split()]
    assert abs(line[-1] - last["n_status"][0] / 48) < 1e-5 and line[-1] > 0.0 and abs(sum(line[1:]) - 1.0) < 1e-5 and abs(line[0] - p0) < 1e-4  # not DAC: p0
    capped = hopping.run(HM.NumpyMfApi(), method="ehrenfest", max_outputs=3, **dict(kw, n_traj=8))
    assert len(capped["records"]) == 3 and capped["steps"] == 2 * capped["output_step"]
    for bad in (dict(decoherence="edc"), dict(reverse_frustrated=True), dict(phase_grid=(8, 8)), dict(method="tully")):
        api = HM.NumpyMfApi()
        with pytest.raises(ValueError):
            hopping.run(api, **{"method": "ehrenfest", **RUN, **bad})
        assert api.calls == []  # refused before anything ran


SCAN = dict(model=hopping.DAC, num_pes=2, momenta=[16.0, 24.0, 30.0], n_per_group=4, seed=1, dt=[2.0, 2.0, 1.0], x0=X0, xmin=LEFT, xmax=RIGHT)


@pytest.mark.parametrize("fixed", [True, False])
def test_scan_until_nobody_runs(tmp_path, fixed):
    api = HM.NumpyMfApi()
    res = hopping.scan(api, fixed=fixed, chunk_steps=128, out_dir=str(tmp_path), method="ehrenfest", **SCAN)
    assert res["method"] == "ehrenfest" and res["stop"] is not None and "NO TRAJECTORY IS RUNNING" in res["stop"]
    assert res["steps"] % 128 == 0 and 0 < res["steps"] <= res["max_steps"]
    calls = api.calls
    assert calls[0] == ("sample_groups", 3, 4) and calls[1] == ("observe_groups_mf",) and len(calls) == 2 + 2 * (res["steps"] // 128)
    assert calls[2::2] == [("evolve_groups_mf", 128)] * (res["steps"] // 128) and all(c == ("observe_groups_mf",) for c in calls[3::2])
    assert res["rows"].shape == (3, 12) and res["hop_counts"] is None and not res["hops"].any() and not res["frustrated"].any()
    pot = HN.builtin(HN.DAC, 2)
    start = HS.sample_groups(pot, 2, 4, 1, [[s["x0"], s["p0"], 0.0 if fixed else s["sigma_x"], 0.0 if fixed else s["sigma_p"]] for s in res["setups"]])
    for g, sl in enumerate(HS.slices(3, 4)):  # every group is the plain call on its slice
        end, _ = HM.evolve(pot, tuple(a[sl] for a in start), MASS, SCAN["dt"][g], res["steps"], LEFT, RIGHT)
        assert np.array_equal(res["rows"][g], HM.observe(pot, end, MASS))
    if fixed:  # nothing is random: the trajectories of a group are one trajectory
        assert all(len(np.unique(res["state"][0][sl])) == 1 for sl in HS.slices(3, 4))
    weights = res["rows"][:, :6].reshape(3, 3, 2)
    assert np.array_equal(res["scattered"], weights[:, 1:] / 4) and not res["running"].any()
    first = HM.observe_groups(pot, start, 4, MASS)
    assert np.array_equal(res["energy_drift"], (res["rows"][:, -1] - first[:, -1]) / 4) and 0.0 < np.abs(res["energy_drift"]).max() < 1e-3
    lines = parse(tmp_path / "scan.txt")  # head, 4 fractions, running, their 5 bounds on the standard error, hops, frustrated, drift
    assert len(lines) == 3 and all(len(line) == 1 + 5 + 5 + 3 for line in lines)
    for g, line in enumerate(lines):
        f = np.array([*res["scattered"][g].reshape(-1), res["running"][g]])
        want = [np.log(res["setups"][g]["p0"] ** 2 / 2.0 / MASS), *f, *np.sqrt(f * (1.0 - f) / 4), 0.0, 0.0, res["energy_drift"][g]]
        assert np.allclose(line, want, rtol=1e-5, atol=1e-300) and abs(f.sum() - 1.0) < 1e-12
        assert np.array_equal(res["stderr"][g], np.sqrt(f * (1.0 - f) / 4))


def test_scan_stops_at_max_steps_and_what_it_refuses():
    res = hopping.scan(HM.NumpyMfApi(), fixed=False, chunk_steps=64, max_steps=200, method="ehrenfest", **SCAN)
    assert res["stop"] is None and res["steps"] == 200 and res["running"].sum() > 0
    api = HM.NumpyMfApi()
    other = hopping.scan(api, fixed=False, chunk_steps=77, max_steps=200, method="ehrenfest", **SCAN)
    assert [c for c in api.calls if c[0] == "evolve_groups_mf"] == [("evolve_groups_mf", 77), ("evolve_groups_mf", 77), ("evolve_groups_mf", 46)]
    assert same_bits(tuple(res["state"][q] for q in (0, 1, 2, 4)), tuple(other["state"][q] for q in (0, 1, 2, 4))) and res["lines"] == other["lines"]
    one = hopping.scan(HM.NumpyMfApi(), **dict(SCAN, n_per_group=1, max_steps=200, method="ehrenfest"))  # fixed=True: a group of one is enough
    four = hopping.scan(HM.NumpyMfApi(), **dict(SCAN, max_steps=200, method="ehrenfest"))
    assert np.allclose(one["scattered"], four["scattered"], rtol=1e-12, atol=0) and np.allclose(one["running"], four["running"], rtol=1e-12)
    for bad in (dict(decoherence="edc"), dict(reverse_frustrated=True), dict(method="tully")):
        api = HM.NumpyMfApi()
        with pytest.raises(ValueError):
            hopping.scan(api, **{"method": "ehrenfest", **SCAN, **bad})
        assert api.calls == []


def test_the_default_method_makes_the_calls_it_made():
    """method="fssh" is the call without method, call for call and bit for bit, on an api that knows nothing of the mean-field methods"""
    runs = []
    for kw in ({}, dict(method="fssh")):
        api = HN.NumpyHopApi()
        res = hopping.run(api, **RUN, **kw)
        runs.append((api.calls, res))
    assert runs[0][0] == runs[1][0] and len(runs[0][0]) > 4 and runs[0][1]["scattering_line"] == runs[1][1]["scattering_line"]
    assert same_bits(runs[0][1]["state"], runs[1][1]["state"]) and runs[1][1]["method"] == "fssh"
    scans = []
    for kw in ({}, dict(method="fssh")):
        api = HS.NumpyScanApi()
        res = hopping.scan(api, fixed=False, chunk_steps=128, max_steps=256, **SCAN, **kw)
        scans.append((api.calls, res))
    assert scans[0][0] == scans[1][0] == [("sample_groups", 3, 4), ("observe_groups",), ("evolve_groups", 0, 128), ("observe_groups",),
                                          ("evolve_groups", 128, 128), ("observe_groups",)]
    assert scans[0][1]["lines"] == scans[1][1]["lines"] and np.array_equal(scans[0][1]["hop_counts"], scans[1][1]["hop_counts"])
