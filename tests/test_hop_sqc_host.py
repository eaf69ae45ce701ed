"""CPU: the numpy restatement of the symmetrical quasi-classical trajectories (tests/hop_sqc_numpy.py), which the GPU tests lean on,
hopping.unpack_sqc, the drivers hopping.run and hopping.scan with method="sqc" on the numpy stand-in api, and the new symbols of the built
library (the test here that fails without the feature)."""
import re
from pathlib import Path

import numpy as np
import pytest

import gaussian_process_liouville_equation_amd as pkg
from gaussian_process_liouville_equation_amd import _capi, hopping
from tests import hop_mf_numpy as HM
from tests import hop_numpy as HN
from tests import hop_scan_numpy as HS
from tests import hop_sqc_numpy as HQ

MASS, X0, LEFT, RIGHT = 2000.0, -4.0, -6.0, 6.0
FAR = 1e3
WINDOWS = [HQ.SQUARE, HQ.TRIANGLE]
NAMES = ("hop_sample_sqc", "hop_sample_groups_sqc", "hop_evolve_sqc", "hop_evolve_groups_sqc", "hop_observe_sqc", "hop_observe_groups_sqc")


def ensemble(potential, num_pes, n, p0, window, seed=11, surface0=0, dtype=np.float64, gamma=None):
    return HQ.sample(potential, num_pes, n, seed, X0, p0, 1.0 / (2.0 * p0 / 20.0), p0 / 20.0, surface0, window, gamma, dtype=dtype)


def same_bits(a, b):
    return all(np.array_equal(u, v) and u.dtype == v.dtype for u, v in zip(a, b))


def test_the_library_exports_and_the_binding_declares_the_six_entry_points():
    lib = pkg.load_library()  # no HIP call at load time: works without a GPU
    text = (Path(__file__).resolve().parent.parent / "include" / "gple.h").read_text()
    for name in NAMES:
        assert name in _capi.GPLE_SYMBOLS
        f = getattr(lib, "gple_" + name)
        assert f.argtypes is not None and len(f.argtypes) == len(_capi.SIGNATURES[name][1])
        assert hasattr(_capi.Api, name)
        assert re.search(r"\bint\s+gple_%s\s*\(" % name, text)
    assert re.search(r"GPLE_TIMER_HOP_SQC\s*=\s*16\b", text) and _capi.TIMER_HOP_SQC == 16
    assert re.search(r"#define\s+GPLE_HOP_WINDOW_SQUARE\s+0\b", text) and re.search(r"#define\s+GPLE_HOP_WINDOW_TRIANGLE\s+1\b", text)
    assert (_capi.HOP_WINDOW_SQUARE, _capi.HOP_WINDOW_TRIANGLE) == (HQ.SQUARE, HQ.TRIANGLE) == (0, 1)
    assert _capi.HOP_WINDOW_GAMMA[0] == HQ.GAMMA[0] == (np.sqrt(3.0) - 1.0) / 2.0 and _capi.HOP_WINDOW_GAMMA[1] == HQ.GAMMA[1] == 1.0 / 3.0
    assert callable(hopping.unpack_sqc) and hopping.SQC == "sqc"


@pytest.mark.parametrize("window", WINDOWS)
def test_the_sample_shares_x_and_p_with_the_other_samples(window):
    pot = HN.builtin(HN.DAC, 2)
    plain = HN.sample(pot, 2, 200, 5, X0, 10.0, 1.0, 0.5, 1, 17)
    got = HQ.sample(pot, 2, 200, 5, X0, 10.0, 1.0, 0.5, 1, window, None, 17)
    assert same_bits((got[0], got[1], got[3], got[4]), (plain[0], plain[1], plain[3], plain[4])) and (got[3] == 1).all()
    packets = [[X0, 10.0, 1.0, 0.5], [X0, 12.0, 0.0, 0.6], [-3.0, 14.0, 0.5, 0.0]]
    plain = HS.sample_groups(pot, 2, 30, 5, packets, 0, 4)
    got = HQ.sample_groups(pot, 2, 30, 5, packets, 0, window, None, 4)
    assert same_bits((got[0], got[1], got[3], got[4]), (plain[0], plain[1], plain[3], plain[4])) and (got[0][30:60] == X0).all() and (got[1][60:] == 14.0).all()
    for g, sl in enumerate(HS.slices(3, 30)):  # a group with both sigmas positive is the plain sample at its offset
        if packets[g][2] > 0 and packets[g][3] > 0:
            assert same_bits(tuple(a[sl] for a in got), HQ.sample(pot, 2, 30, 5, *packets[g], 0, window, None, 4 + 30 * g))
    part = HQ.sample(pot, 2, 150, 5, X0, 10.0, 1.0, 0.5, 1, window, None, 17 + 50)  # a slice with its offset
    assert same_bits(part, tuple(a[50:] for a in HQ.sample(pot, 2, 200, 5, X0, 10.0, 1.0, 0.5, 1, window, None, 17)))


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("N,model,surface0", [(2, HN.DAC, 0), (2, HN.ECR, 1), (3, HN.TSAC, 0), (3, HN.TSAC, 1), (3, HN.TSAC, 2)])
def test_every_start_lies_in_its_window_with_the_expected_mean(window, N, model, surface0):
    n, gamma = 65536, HQ.GAMMA[window]
    u, _ = HQ.level_uniforms(np.arange(n), N, 3, np.float64)
    e = HQ.start_energies(u, surface0, window, gamma)
    assert (HQ.window_of(e, window, gamma) == surface0).all()
    occupied = np.arange(N) == surface0
    want = np.where(occupied, 1.0, 0.0) + gamma if window == HQ.SQUARE else np.where(occupied, 2.0 - N / (N + 1.0), N / (2.0 * (N + 1.0)))
    if window == HQ.TRIANGLE:
        assert np.allclose(want, [4.0 / 3.0, 1.0 / 3.0] if N == 2 else [5.0 / 4.0, 3.0 / 8.0, 3.0 / 8.0]) or surface0 != 0
    err = np.abs(e.mean(axis=0) - want) / (e.std(axis=0, ddof=1) / np.sqrt(n))
    print(f"sqc start window {window} N {N} from {surface0}: mean e {e.mean(axis=0)}, expected {want}, standard errors off {err}")
    assert (err <= 6.0).all()
    # the amplitudes carry these energies in the adiabatic representation
    pot = HN.builtin(model, N)
    state = ensemble(pot, N, 512, 10.0, window, seed=3, surface0=surface0)
    got, _ = HQ.energies(pot, state)
    assert np.abs(got - e[:512]).max() <= 1e-14 and (HQ.window_of(got, window, gamma) == surface0).all()


@pytest.mark.parametrize("window", WINDOWS)
def test_the_norm_is_conserved_and_is_not_one(window):
    pot = HN.builtin(HN.DAC, 2)
    start = ensemble(pot, 2, 64, 16.0, window)
    (x, p, b, surface, status), _ = HQ.evolve(pot, start, MASS, 1.0, 1000, -FAR, FAR, HQ.GAMMA[window])
    before, after = HM.norms(start[2]).sum(axis=1), HM.norms(b).sum(axis=1)
    worst = np.abs(after - before).max()
    print(f"sqc window {window}: | sum |b|^2 - its start | after 1000 steps {worst:.3g}; the norms lie in [{before.min():.3f}, {before.max():.3f}]")
    assert (status == 0).all() and worst <= 1e-12 and np.abs(before - 1.0).min() > 1e-6


@pytest.mark.parametrize("window", WINDOWS)
def test_the_integrator_is_of_second_order_in_the_mapping_hamiltonian(window):
    """The mean-field test's rule on H = p^2 / 2m + b^dagger V b - gamma tr V: DAC at p0 = 16, where tr V != 0, so that a wrong sign of the
    gamma term in the force shows as a drift that does not fall"""
    pot = HN.builtin(HN.DAC, 2)
    gamma = HQ.GAMMA[window]
    state = ensemble(pot, 2, 64, 16.0, window)
    worst = [HQ.evolve(pot, state, MASS, dt, int(1000 / dt), -FAR, FAR, gamma)[1]["drift"].max() for dt in (2.0, 1.0, 0.5)]
    ratios = [worst[0] / worst[1], worst[1] / worst[2]]
    print("sqc window %d: deviation of H %.3g %.3g %.3g, ratios %.4f %.4f" % (window, *worst, *ratios))
    assert all(3.9 <= r <= 4.1 for r in ratios), ratios


@pytest.mark.parametrize("model,N", [(HN.DAC, 2), (HN.SAC, 2), (HN.TSAC, 3)])
def test_the_force_is_minus_the_derivative_of_the_hamiltonian(model, N):
    """f against a central difference of H in x at fixed b, in long double with h = 1e-6: the truncation error is h^2 / 6 |H'''| ~ 1e-14, the
    rounding error 1e-19 / h"""
    pot = HN.builtin(model, N)
    rng = np.random.default_rng(5)
    x = np.linspace(-5.0, 5.0, 200).astype(np.longdouble)
    b = (rng.normal(size=(200, N)) + 1j * rng.normal(size=(200, N))).astype(np.clongdouble)
    p, h, gamma = np.zeros(200, dtype=np.longdouble), np.longdouble(1e-6), 0.3660254037844386
    H = lambda xx: HQ.hamiltonian(pot(xx)[0], p, b, MASS, gamma)
    want = -(H(x + h) - H(x - h)) / (2 * h)
    got = HQ.force(pot(x)[1], b, gamma)
    wrong = HM.force(pot(x)[1], b) + gamma * HQ.trace(pot(x)[1])
    scale = np.abs(pot(x)[1]).sum(axis=(1, 2)).max() * float(HM.norms(b).sum(axis=1).max())
    worst = float(np.abs(got - want).max() / scale)
    print(f"sqc force {model}: relative difference to the central difference {worst:.3g}; with the other sign {float(np.abs(wrong - want).max() / scale):.3g}")
    assert worst <= 1e-10
    if model == HN.DAC:  # the one model here with tr V != 0: on SAC and TSAC the gamma term vanishes and this test cannot see its sign
        assert np.abs(wrong - want).max() / scale > 1e-3


def test_gamma_zero_is_the_mean_field_step_bit_for_bit():
    pot = HN.builtin(HN.DAC, 2)
    state = HN.sample(pot, 2, 48, 11, X0, 10.0, 1.0, 0.5)
    assert same_bits(HQ.evolve(pot, state, MASS, 2.0, 900, LEFT, RIGHT, 0.0)[0], HM.evolve(pot, state, MASS, 2.0, 900, LEFT, RIGHT)[0])


@pytest.mark.parametrize("model,N,p0,dt,steps", [(HN.DAC, 2, 10.0, 2.0, 600), (HN.TSAC, 3, 10.0, 4.0, 300)])
def test_the_sign_of_the_eigenvectors_changes_nothing(model, N, p0, dt, steps):
    pot = HN.builtin(model, N)
    state = ensemble(pot, N, 96, p0, HQ.TRIANGLE)
    plain, _ = HQ.evolve(pot, state, MASS, dt, steps, LEFT, RIGHT, 1.0 / 3.0)
    flipped, _ = HQ.evolve(pot, state, MASS, dt, steps, LEFT, RIGHT, 1.0 / 3.0, flip=True)
    assert same_bits(plain, flipped) and (plain[4] != 0).any()


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("N", [2, 3])
def test_the_windows_are_disjoint_and_every_trajectory_is_counted_once(window, N):
    gamma = HQ.GAMMA[window]
    rng = np.random.default_rng(9)
    e = rng.uniform(0.0, 2.2, size=(20000, N))
    inside = np.zeros((len(e), N), dtype=bool)
    for k, tests in enumerate(HQ._comparisons(e, window, gamma)):
        inside[:, k] = np.all([(left >= edge) if sense > 0 else (left <= edge) for left, edge, sense in tests], axis=0)
    assert inside.sum(axis=1).max() == 1 and (inside.sum(axis=0) > 20).all() and (inside.sum(axis=1) == 0).sum() > 20
    found = HQ.window_of(e, window, gamma)
    assert np.array_equal(found >= 0, inside.any(axis=1)) and all((found[inside[:, k]] == k).all() for k in range(N))
    # the sums: windowed + none = the count of the status; a status out of range adds nowhere
    pot = HN.builtin(HN.DAC if N == 2 else HN.TSAC, N)
    state, _ = HQ.evolve(pot, ensemble(pot, N, 120, 10.0, window), MASS, 4.0, 450, LEFT, RIGHT, gamma)
    terms = HQ.observe_terms(pot, state, MASS, window, gamma)
    rec = hopping.unpack_sqc(terms.sum(axis=0), N, 120, gamma)
    assert np.array_equal(rec["counts"].sum(axis=1) + rec["none"], rec["n_status"]) and np.array_equal(rec["n_status"], np.bincount(state[4], minlength=3))
    assert rec["n_status"].sum() == 120 and (rec["n_status"] > 0).sum() >= 2 and rec["none"].sum() > 0 and (terms[:, :3 * N + 6].sum(axis=1) == 2).all()
    odd = state[:4] + (np.where(np.arange(120) < 7, np.where(np.arange(120) % 2 == 0, 3, -1), state[4]).astype(np.int32),)
    skipped = HQ.observe_terms(pot, odd, MASS, window, gamma)
    assert not skipped[:7].any() and np.array_equal(skipped[7:], terms[7:])


def test_evolve_carries_nothing_hidden_and_a_slice_or_a_group_is_the_plain_call():
    pot = HN.builtin(HN.DAC, 2)
    gamma = 1.0 / 3.0
    state = ensemble(pot, 2, 48, 10.0, HQ.TRIANGLE)
    whole, _ = HQ.evolve(pot, state, MASS, 2.0, 900, LEFT, RIGHT, gamma)
    rest, _ = HQ.evolve(pot, HQ.evolve(pot, state, MASS, 2.0, 350, LEFT, RIGHT, gamma)[0], MASS, 2.0, 550, LEFT, RIGHT, gamma)
    assert same_bits(whole, rest) and (whole[4] != 0).any() and (whole[4] == 0).any() and whole[3] is state[3]
    part, _ = HQ.evolve(pot, tuple(a[20:] for a in state), MASS, 2.0, 900, LEFT, RIGHT, gamma)
    assert same_bits(tuple(a[20:] for a in whole), part)
    later, _ = HQ.evolve(pot, whole, MASS, 2.0, 100, LEFT, RIGHT, gamma)  # a finished trajectory is frozen
    done = whole[4] != 0
    assert same_bits(tuple(a[done] for a in later), tuple(a[done] for a in whole))
    dt = np.array([2.0, 1.0, 4.0])
    grouped, _ = HQ.evolve_groups(pot, state, 16, MASS, dt, 300, LEFT, RIGHT, gamma)
    for g, sl in enumerate(HS.slices(3, 16)):
        assert same_bits(tuple(a[sl] for a in grouped), HQ.evolve(pot, tuple(a[sl] for a in state), MASS, dt[g], 300, LEFT, RIGHT, gamma)[0])
    assert same_bits(HQ.evolve_groups(pot, state, 16, MASS, np.full(3, 2.0), 900, LEFT, RIGHT, gamma)[0], whole)
    rows = HQ.observe_groups(pot, grouped, 16, MASS, HQ.TRIANGLE, gamma)
    assert rows.shape == (3, 17) and np.array_equal(rows[1], HQ.observe(pot, tuple(a[16:32] for a in grouped), MASS, HQ.TRIANGLE, gamma))


def test_unpack_sqc_and_the_three_level_layout():
    pot = HN.builtin(HN.TSAC, 3)
    gamma = HQ.GAMMA[HQ.SQUARE]
    state, _ = HQ.evolve(pot, ensemble(pot, 3, 60, 10.0, HQ.SQUARE), MASS, 4.0, 600, LEFT, RIGHT, gamma)
    rec = hopping.unpack_sqc(HQ.observe(pot, state, MASS, HQ.SQUARE, gamma), 3, 60, gamma)
    e, E = HQ.energies(pot, state)
    found = HQ.window_of(e, HQ.SQUARE, gamma)
    assert rec["counts"].shape == (3, 3) and rec["n_status"].shape == rec["none"].shape == (3,) and rec["e"].shape == rec["actions"].shape == (3,)
    for status in range(3):
        of = state[4] == status
        assert rec["n_status"][status] == of.sum() and rec["none"][status] == (of & (found < 0)).sum()
        assert np.array_equal(rec["counts"][status], [(of & (found == k)).sum() for k in range(3)])
    assert np.abs(rec["e"] - e.mean(axis=0)).max() < 1e-13 and np.array_equal(rec["actions"], rec["e"] - gamma)
    assert np.array_equal(rec["windowed"], rec["counts"].sum(axis=0) / 60) and rec["unassigned"] == rec["none"].sum() / 60
    assert abs(rec["windowed"].sum() + rec["unassigned"] - 1.0) < 1e-15
    assert abs(rec["x"] - state[0].mean()) < 1e-12 and abs(rec["p"] - state[1].mean()) < 1e-12
    assert abs(rec["E"] - np.mean(state[1] ** 2 / 2.0 / MASS + np.sum((e - gamma) * E, axis=1))) < 1e-12
    assert abs(rec["E"] - HQ.hamiltonian(pot(state[0])[0], state[1], state[2], MASS, gamma).mean()) < 1e-12  # the two forms of H
    with pytest.raises(ValueError):
        hopping.unpack_sqc(np.zeros(20), 3, 60, gamma)
    channels, n_f, lost = hopping.sqc_channels(rec["counts"], rec["n_status"], rec["none"])
    assert n_f == rec["counts"][1:].sum() > 0 and np.array_equal(channels, rec["counts"][1:] / n_f) and lost == rec["none"][1:].sum() / rec["n_status"][1:].sum()
    channels, n_f, lost = hopping.sqc_channels(np.zeros((3, 3)), [60, 0, 0], [60, 0, 0])
    assert n_f == 0 and lost == 0 and not channels.any()


def parse(path):
    return [[float(v) for v in line.split()] for line in open(path)]


RUN = dict(model=hopping.DAC, num_pes=2, ln_energy=-2.0, n_traj=48, seed=4, dt=4.0, x0=X0, xmin=LEFT, xmax=RIGHT)


@pytest.mark.parametrize("window", ["square", "triangle", None])
def test_run_until_nobody_runs(tmp_path, window):
    api = HQ.NumpySqcApi()
    res = hopping.run(api, out_dir=str(tmp_path), method="sqc", **({} if window is None else dict(window=window)), **RUN)
    code = HQ.SQUARE if window == "square" else HQ.TRIANGLE
    gamma = HQ.GAMMA[code]
    assert res["method"] == "sqc" and res["window"] == code and res["gamma"] == gamma and res["stop"] is not None and "NO TRAJECTORY IS RUNNING" in res["stop"]
    step, count = res["output_step"], len(res["records"])
    # one sample, then an observe per output time and an evolve of output_step steps between two of them
    calls = api.calls
    assert calls[0] == ("sample_sqc", 48, code, gamma) and len(calls) == 2 * count
    assert calls[1::2] == [("observe_sqc", code, gamma)] * count and calls[2::2] == [("evolve_sqc", step, gamma)] * (count - 1)
    t, av = parse(tmp_path / "t.txt"), parse(tmp_path / "averages.txt")
    assert len(t) == len(av) == count
    for rec, (tt,), line in zip(res["records"], t, av):
        assert len(line) == 4 + 2 + 2 + 1
        want = [rec["t"], rec["E"], rec["x"], rec["p"], *(rec["counts"].sum(axis=0) / 48), *(rec["e"] - gamma), rec["none"].sum() / 48]
        assert np.allclose([tt] + line, [rec["t"]] + want, rtol=1e-5, atol=1e-300)
    last = res["records"][-1]
    assert last["n_status"][0] == 0 and last["n_status"].sum() == 48
    n_f = last["counts"][1:].sum()
    line = [float(v) for v in res["scattering_line"].split()]
    assert len(line) == 1 + 4 + 1 + 1 and line[5] == 0.0 and abs(sum(line[1:5]) - 1.0) < 1e-5 and abs(line[0] + 2.0) < 1e-5
    assert np.array_equal(res["scattered"], last["counts"][1:] / n_f) and abs(line[6] - last["none"][1:].sum() / last["n_status"][1:].sum()) < 1e-5 and 0 < n_f < 48
    assert (np.asarray(res["state"][3]) == 0).all()


def test_run_until_the_total_time_and_what_it_refuses(tmp_path):
    p0 = float(np.sqrt(2.0 * MASS * np.exp(-2.0)))
    kw = dict(RUN, model=hopping.SAC, dt=8.0, sigma_p=p0 / 2.0)  # a packet as wide as its momentum: some trajectories crawl
    res = hopping.run(HQ.NumpySqcApi(), out_dir=str(tmp_path), method="sqc", window="square", gamma=0.25, **kw)
    assert res["stop"] is None and res["steps"] + res["output_step"] > res["total_step"] >= res["steps"] and res["gamma"] == 0.25
    last = res["records"][-1]
    assert last["n_status"][0] > 0 and last["n_status"].sum() == 48
    line = [float(v) for v in res["scattering_line"].split()]
    assert abs(line[5] - last["n_status"][0] / 48) < 1e-5 and line[5] > 0.0 and abs(line[0] - p0) < 1e-4  # not DAC: p0
    early = hopping.run(HQ.NumpySqcApi(), method="sqc", max_outputs=1, **RUN)  # nobody has finished: N_f = 0, the channels are 0
    assert len(early["records"]) == 1 and [float(v) for v in early["scattering_line"].split()][1:] == [0.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    bad = [dict(decoherence="edc"), dict(reverse_frustrated=True), dict(phase_grid=(8, 8)), dict(method="tully"), dict(window="circle"), dict(gamma=-0.1),
           dict(gamma=float("nan")), dict(window="square", gamma=0.5), dict(window="square", gamma=0.0), dict(method="fssh", window="square"),
           dict(method="ehrenfest", gamma=0.3), dict(method="fssh", gamma=0.3), dict(method="ehrenfest", window="triangle")]
    for kw in bad:
        api = HQ.NumpySqcApi()
        with pytest.raises(ValueError):
            hopping.run(api, **{"method": "sqc", **RUN, **kw})
        assert api.calls == [], kw  # refused before anything ran
    assert hopping.run(HQ.NumpySqcApi(), method="sqc", gamma=0.0, max_outputs=1, **RUN)["gamma"] == 0.0  # the triangle takes any gamma >= 0


SCAN = dict(model=hopping.DAC, num_pes=2, momenta=[16.0, 24.0, 30.0], n_per_group=12, seed=1, dt=[2.0, 2.0, 1.0], x0=X0, xmin=LEFT, xmax=RIGHT)


@pytest.mark.parametrize("fixed", [True, False])
@pytest.mark.parametrize("window", ["square", "triangle"])
def test_scan_until_nobody_runs(tmp_path, fixed, window):
    api = HQ.NumpySqcApi()
    res = hopping.scan(api, fixed=fixed, chunk_steps=128, out_dir=str(tmp_path), method="sqc", window=window, **SCAN)
    code = HQ.SQUARE if window == "square" else HQ.TRIANGLE
    gamma = HQ.GAMMA[code]
    assert res["method"] == "sqc" and res["stop"] is not None and "NO TRAJECTORY IS RUNNING" in res["stop"] and res["steps"] % 128 == 0
    chunks = res["steps"] // 128
    calls = api.calls
    assert calls[0] == ("sample_groups_sqc", 3, 12, code, gamma) and len(calls) == 2 + 2 * chunks
    assert calls[1::2] == [("observe_groups_sqc", code, gamma)] * (1 + chunks) and calls[2::2] == [("evolve_groups_sqc", 128, gamma)] * chunks
    assert res["rows"].shape == (3, 17) and res["hop_counts"] is None and not res["hops"].any() and not res["frustrated"].any()
    pot = HN.builtin(HN.DAC, 2)
    packets = [[s["x0"], s["p0"], 0.0 if fixed else s["sigma_x"], 0.0 if fixed else s["sigma_p"]] for s in res["setups"]]
    start = HQ.sample_groups(pot, 2, 12, 1, packets, 0, code, gamma)
    for g, sl in enumerate(HS.slices(3, 12)):  # every group is the plain call on its slice
        end, _ = HQ.evolve(pot, tuple(a[sl] for a in start), MASS, SCAN["dt"][g], res["steps"], LEFT, RIGHT, gamma)
        assert np.array_equal(res["rows"][g], HQ.observe(pot, end, MASS, code, gamma))
    if fixed:  # the packet is a point, the actions and angles are still drawn
        assert all(len(np.unique(res["state"][0][sl])) > 1 for sl in HS.slices(3, 12)) and all(len(np.unique(start[0][sl])) == 1 for sl in HS.slices(3, 12))
    counts, none = res["rows"][:, :6].reshape(3, 3, 2), res["rows"][:, 9:12]
    n_f = counts[:, 1:].sum(axis=(1, 2))
    assert (n_f > 0).all() and np.array_equal(res["scattered"], counts[:, 1:] / n_f[:, None, None]) and not res["running"].any()
    first = HQ.observe_groups(pot, start, 12, MASS, code, gamma)
    assert np.array_equal(res["energy_drift"], (res["rows"][:, -1] - first[:, -1]) / 12) and 0.0 < np.abs(res["energy_drift"]).max() < 1e-3
    lines = parse(tmp_path / "scan.txt")  # head, 4 channels, running, their 5 standard errors, hops, frustrated, drift, unassigned finished
    assert len(lines) == 3 and all(len(line) == 1 + 5 + 5 + 3 + 1 for line in lines)
    for g, line in enumerate(lines):
        f = res["scattered"][g].reshape(-1)
        want = [np.log(res["setups"][g]["p0"] ** 2 / 2.0 / MASS), *f, 0.0, *np.sqrt(f * (1.0 - f) / n_f[g]), 0.0, 0.0, 0.0, res["energy_drift"][g], none[g, 1:].sum() / 12]
        assert np.allclose(line, want, rtol=1e-5, atol=1e-300) and abs(f.sum() - 1.0) < 1e-12


def test_scan_stops_at_max_steps_and_what_it_refuses():
    res = hopping.scan(HQ.NumpySqcApi(), fixed=False, chunk_steps=64, max_steps=200, method="sqc", **SCAN)
    assert res["stop"] is None and res["steps"] == 200 and res["running"].sum() > 0 and res["window"] == HQ.TRIANGLE
    api = HQ.NumpySqcApi()
    other = hopping.scan(api, fixed=False, chunk_steps=77, max_steps=200, method="sqc", **SCAN)
    assert [c[:2] for c in api.calls if c[0] == "evolve_groups_sqc"] == [("evolve_groups_sqc", 77), ("evolve_groups_sqc", 77), ("evolve_groups_sqc", 46)]
    assert same_bits(tuple(res["state"][q] for q in (0, 1, 2, 4)), tuple(other["state"][q] for q in (0, 1, 2, 4))) and res["lines"] == other["lines"]
    none = hopping.scan(HQ.NumpySqcApi(), max_steps=0, method="sqc", **SCAN)  # nobody has finished: the channel columns and their errors are 0
    assert not none["scattered"].any() and not none["stderr"][:, :4].any() and (none["running"] == 1).all() and not none["unassigned_finished"].any()
    for bad in (dict(decoherence="edc"), dict(reverse_frustrated=True), dict(method="tully"), dict(window="circle"), dict(window="square", gamma=0.7),
                dict(method="fssh", window="triangle"), dict(method="ehrenfest", gamma=0.2)):
        api = HQ.NumpySqcApi()
        with pytest.raises(ValueError):
            hopping.scan(api, **{"method": "sqc", **SCAN, **bad})
        assert api.calls == [], bad


def test_the_other_methods_make_the_calls_they_made():
    """method="fssh" and "ehrenfest" on stand-ins that know nothing of the six new methods: the recorded calls are those of the parent commit"""
    api = HN.NumpyHopApi()
    res = hopping.run(api, **RUN)
    count, step = len(res["records"]), res["output_step"]
    assert not any(hasattr(api, name) for name in NAMES) and "window" not in res
    assert api.calls == [("sample", 48)] + [c for k in range(count - 1) for c in (("observe",), ("evolve", k * step, step))] + [("observe",)]
    api = HM.NumpyMfApi()
    res = hopping.run(api, method="ehrenfest", **RUN)
    count = len(res["records"])
    assert not any(hasattr(api, name) for name in NAMES)
    assert api.calls == [("sample", 48)] + [c for _ in range(count - 1) for c in (("observe_mf",), ("evolve_mf", step))] + [("observe_mf",)]
    api = HS.NumpyScanApi()
    hopping.scan(api, fixed=False, chunk_steps=128, max_steps=256, **dict(SCAN, n_per_group=4))
    assert api.calls == [("sample_groups", 3, 4), ("observe_groups",), ("evolve_groups", 0, 128), ("observe_groups",), ("evolve_groups", 128, 128), ("observe_groups",)]
    api = HM.NumpyMfApi()
    hopping.scan(api, fixed=False, chunk_steps=128, max_steps=256, method="ehrenfest", **dict(SCAN, n_per_group=4))
    assert api.calls == [("sample_groups", 3, 4), ("observe_groups_mf",), ("evolve_groups_mf", 128), ("observe_groups_mf",), ("evolve_groups_mf", 128),
                         ("observe_groups_mf",)]
