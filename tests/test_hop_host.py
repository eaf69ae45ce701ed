"""CPU: the numpy restatement of the surface hopping step (tests/hop_numpy.py), which the GPU tests lean on, the driver hopping.run on a numpy
stand-in api, and the new symbols of the built library (the one test here that fails without the feature)."""
import numpy as np
import pytest

import gaussian_process_liouville_equation_amd as pkg
from gaussian_process_liouville_equation_amd import _capi, exact, hopping
from tests import hop_numpy as HN

MASS = 2000.0


def ensemble(potential, num_pes, n, p0, seed=11, surface0=0, dtype=np.float64, x0=-4.0):
    return HN.sample(potential, num_pes, n, seed, x0, p0, 1.0 / (2.0 * p0 / 20.0), p0 / 20.0, surface0=surface0, dtype=dtype)


@pytest.mark.parametrize("N", [2, 3])
def test_jacobi_against_eigh(N):
    rng = np.random.default_rng(N)
    A = rng.uniform(-0.5, 0.5, (512, N, N))
    A = 0.5 * (A + np.swapaxes(A, 1, 2))
    A[:8, 0, 1] = A[:8, 1, 0] = 0.0  # pairs that are not rotated
    lam, W = HN.jacobi(A)
    ref = np.linalg.eigvalsh(A)
    assert np.abs(lam - ref).max() <= 1e-14
    assert np.abs(np.swapaxes(W, 1, 2) @ W - np.eye(N)).max() <= 1e-14
    assert np.abs(A @ W - W * lam[:, None, :]).max() <= 1e-14
    # eigenvectors up to sign where the levels are well apart
    _, V = np.linalg.eigh(A)
    apart = np.min(np.diff(ref, axis=1), axis=1) > 0.05
    overlap = np.abs(np.einsum("mik,mik->mk", W, V))
    assert apart.sum() > 100 and np.abs(overlap[apart] - 1.0).max() <= 1e-13


def test_a_decoupled_level_keeps_exact_zeros():
    pot = HN.builtin(HN.DAC, 3)
    x = np.linspace(-3.0, 3.0, 41)
    _, E, C, F = HN.states(x, pot)
    spectator = np.argmax(np.abs(C[:, 2, :]), axis=1)  # the column that is the third diabat
    for m, k in enumerate(spectator):
        others = [j for j in range(3) if j != k]
        assert np.all(C[m, 2, others] == 0.0) and np.all(C[m, :2, k] == 0.0) and abs(C[m, 2, k]) == 1.0
        assert np.all(F[m, k, others] == 0.0)


def test_the_amplitudes_stay_normalised():
    pot = HN.builtin(HN.DAC, 2)
    state = ensemble(pot, 2, 64, 16.0)
    (x, p, b, surface, status), diag = HN.evolve(pot, state, 11, MASS, 1.0, 0, 1000, -1e3, 1e3)
    assert (status == 0).all() and diag["hops"].sum() >= 10
    assert np.abs(np.sum(np.abs(b) ** 2, axis=1) - 1.0).max() <= 1e-12


def energies(potential, state):
    x, p, _, surface, _ = state
    _, E, _, _ = HN.states(x, potential)
    return p * p / 2.0 / MASS + E[np.arange(len(x)), surface]


def test_the_energy_drift_is_second_order_in_dt():
    """Velocity Verlet on one surface: the largest deviation of p^2 / 2m + E_a along a trajectory falls by a factor of 4 when dt is halved.  DAC
    (smooth, unlike the models with sgn(x) in them) at p0 = 16 through both crossings; the two runs draw different numbers, so the statement
    is made for the trajectories that never hop in either, which follow the same path in both: most of them"""
    pot = HN.builtin(HN.DAC, 2)
    n = 64
    state = ensemble(pot, 2, n, 16.0)
    e0 = energies(pot, state)
    worst, quiet = {}, np.ones(n, dtype=bool)
    for halvings, dt in ((0, 2.0), (1, 1.0)):
        s, dev, first = state, np.zeros(n), 0
        for _ in range(25):
            s, diag = HN.evolve(pot, s, 11, MASS, dt, first, 20 << halvings, -1e3, 1e3)
            quiet &= (diag["hops"] == 0) & (diag["frustrated"] == 0)
            first += 20 << halvings
            dev = np.maximum(dev, np.abs(energies(pot, s) - e0))
        worst[halvings] = dev
    ratio = worst[0][quiet] / worst[1][quiet]
    print("energy drift ratio over %d trajectories: %.3f ... %.3f" % (quiet.sum(), ratio.min(), ratio.max()))
    assert quiet.sum() >= n // 2 and worst[1][quiet].min() > 1e-12 and (ratio > 3.0).all() and (ratio < 5.0).all()


def test_a_hop_conserves_the_energy():
    """DAC at p0 = 16: the surfaces are 0.02 ... 0.05 apart where the hops happen; with dt = 1/4 the energy of every trajectory, hops included,
    moves by the integrator's error alone"""
    pot = HN.builtin(HN.DAC, 2)
    state = ensemble(pot, 2, 32, 16.0)
    end, diag = HN.evolve(pot, state, 11, MASS, 0.25, 0, 3200, -1e3, 1e3)
    assert diag["hops"].sum() >= 5
    assert np.abs(energies(pot, end) - energies(pot, state)).max() <= 1e-7


@pytest.mark.parametrize("model,N,p0,dt,steps,surface0", [(HN.DAC, 2, 10.0, 2.0, 600, 0), (HN.TSAC, 3, 10.0, 4.0, 200, 1)])
def test_the_sign_of_the_eigenvectors_changes_nothing(model, N, p0, dt, steps, surface0):
    pot = HN.builtin(model, N)
    state = ensemble(pot, N, 96, p0, surface0=surface0)
    plain, d0 = HN.evolve(pot, state, 11, MASS, dt, 0, steps, -6.0, 6.0)
    flipped, d1 = HN.evolve(pot, state, 11, MASS, dt, 0, steps, -6.0, 6.0, flip=True)
    wide = tuple(a.astype(np.longdouble) if a.dtype == np.float64 else a.astype(np.clongdouble) if a.dtype == np.complex128 else a for a in state)
    exact_run, _ = HN.evolve(pot, wide, 11, MASS, dt, 0, steps, -6.0, 6.0)
    assert d0["hops"].sum() >= 10
    assert np.array_equal(d0["hops"], d1["hops"]) and np.array_equal(d0["frustrated"], d1["frustrated"])
    assert np.array_equal(plain[3], flipped[3]) and np.array_equal(plain[4], flipped[4])
    for q in (0, 1):
        D = np.abs(plain[q] - exact_run[q]).max()
        assert np.abs(plain[q] - flipped[q]).max() <= HN.tolerance(D, plain[q])
    # the diabatic amplitudes do not see the flip either
    assert np.abs(plain[2] - flipped[2]).max() <= HN.tolerance(np.abs(plain[2] - exact_run[2]).max(), plain[2])


def test_the_sample_is_the_gaussian():
    n, x0, p0, sx, sp = 1 << 16, -4.0, 16.0, 0.625, 0.8
    x, p, b, surface, status = HN.sample(HN.builtin(HN.DAC, 2), 2, n, 5, x0, p0, sx, sp)
    for v, mean, sigma in ((x, x0, sx), (p, p0, sp)):
        assert abs(v.mean() - mean) <= 4.0 * sigma / np.sqrt(n)
        assert abs(v.var(ddof=1) - sigma ** 2) <= 4.0 * sigma ** 2 * np.sqrt(2.0 / (n - 1))
    assert abs(np.mean((x - x0) * (p - p0))) <= 4.0 * sx * sp / np.sqrt(n)
    assert (surface == 0).all() and (status == 0).all() and np.abs(np.sum(np.abs(b) ** 2, axis=1) - 1.0).max() <= 8 * np.finfo(np.float64).eps
    # a slice has the bits it has inside the whole
    part = HN.sample(HN.builtin(HN.DAC, 2), 2, 100, 5, x0, p0, sx, sp, trajectory_offset=1000)
    assert np.array_equal(part[0], x[1000:1100]) and np.array_equal(part[1], p[1000:1100])


def test_evolve_carries_nothing_hidden():
    pot = HN.builtin(HN.DAC, 2)
    state = ensemble(pot, 2, 48, 10.0)
    whole, _ = HN.evolve(pot, state, 3, MASS, 2.0, 0, 400, -6.0, 6.0)
    half, _ = HN.evolve(pot, state, 3, MASS, 2.0, 0, 150, -6.0, 6.0)
    rest, _ = HN.evolve(pot, half, 3, MASS, 2.0, 150, 250, -6.0, 6.0)
    assert all(np.array_equal(a, b) for a, b in zip(whole, rest))
    part, _ = HN.evolve(pot, tuple(a[20:] for a in state), 3, MASS, 2.0, 0, 400, -6.0, 6.0, trajectory_offset=20)
    assert all(np.array_equal(a[20:], b) for a, b in zip(whole, part))


def parse(path):
    return [[float(v) for v in line.split()] for line in open(path)]


def check_files(res, out_dir, num_pes):
    t = parse(out_dir / "t.txt")
    av = parse(out_dir / "averages.txt")
    assert len(t) == len(av) == len(res["records"])
    for rec, (tt,), line in zip(res["records"], t, av):
        want = [rec["t"], rec["E"], rec["x"], rec["p"], *(rec["counts"].sum(axis=0) / res["n_traj"]), *rec["populations"]]
        assert len(line) == 4 + 2 * num_pes
        assert np.allclose([tt] + line, [rec["t"]] + want, rtol=1e-5, atol=1e-300)


def test_driver_until_nobody_runs(tmp_path):
    api = HN.NumpyHopApi()
    res = hopping.run(api, model=hopping.DAC, num_pes=2, ln_energy=-2.0, n_traj=48, seed=4, out_dir=str(tmp_path), dt=4.0, x0=-4.0, xmin=-6.0, xmax=6.0)
    s = res["setup"]
    assert res["stop"] is not None and "NO TRAJECTORY IS RUNNING" in res["stop"]
    assert res["output_step"] == int(s["output_time"] / 4.0) and res["steps"] <= res["total_step"]
    # one sample, then an observe per output time and an evolve of output_step steps between two of them
    calls = api.calls
    assert calls[0] == ("sample", 48) and calls[1] == ("observe",)
    assert calls[2::2] == [("evolve", k * res["output_step"], res["output_step"]) for k in range(len(res["records"]) - 1)]
    assert all(c == ("observe",) for c in calls[3::2])
    check_files(res, tmp_path, 2)
    last = res["records"][-1]
    assert last["counts"].sum() == 48 and last["counts"][hopping.RUNNING].sum() == 0
    line = [float(v) for v in res["scattering_line"].split()]
    assert len(line) == 1 + 2 * 2 + 1 and line[-1] == 0.0 and abs(sum(line[1:]) - 1.0) < 1e-5
    assert abs(line[0] - (-2.0)) < 1e-5  # DAC: ln E, as exact.run's final line
    assert np.array_equal(res["scattered"], last["counts"][1:] / 48)
    # the same head as the DVR flux line's
    assert exact.fmt(np.log(s["p0"] ** 2 / 2.0 / s["mass"])) == res["scattering_line"].split()[0]


def test_driver_until_the_total_time(tmp_path):
    """a packet as wide as its momentum: some trajectories crawl and are still inside when the total time is over"""
    p0 = float(np.sqrt(2.0 * MASS * np.exp(-2.0)))
    res = hopping.run(HN.NumpyHopApi(), model=hopping.SAC, num_pes=2, ln_energy=-2.0, n_traj=48, seed=4, out_dir=str(tmp_path), dt=8.0, x0=-4.0, xmin=-6.0,
                      xmax=6.0, sigma_p=p0 / 2.0, reverse_frustrated=True)
    assert res["stop"] is None and res["steps"] + res["output_step"] > res["total_step"] >= res["steps"]
    last = res["records"][-1]
    assert last["counts"][hopping.RUNNING].sum() > 0 and last["counts"].sum() == 48
    check_files(res, tmp_path, 2)
    line = [float(v) for v in res["scattering_line"].split()]
    assert line[-1] > 0.0 and abs(sum(line[1:]) - 1.0) < 1e-5 and abs(line[0] - p0) < 1e-4  # not DAC: p0
    capped = hopping.run(HN.NumpyHopApi(), model=hopping.SAC, num_pes=2, ln_energy=-2.0, n_traj=8, dt=8.0, x0=-4.0, xmin=-6.0, xmax=6.0, max_outputs=3)
    assert len(capped["records"]) == 3 and capped["steps"] == 2 * capped["output_step"]
    with pytest.raises(ValueError):
        hopping.run(HN.NumpyHopApi(), n_traj=8, dt=1e6)


def test_unpack_and_the_three_level_layout():
    pot = HN.builtin(HN.TSAC, 3)
    state = ensemble(pot, 3, 40, 10.0, surface0=1)
    state, _ = HN.evolve(pot, state, 2, MASS, 4.0, 0, 250, -6.0, 6.0)
    rec = hopping.unpack(HN.observe(pot, state, MASS), 3, 40)
    for status in range(3):
        for k in range(3):
            assert rec["counts"][status, k] == np.sum((state[4] == status) & (state[3] == k))
    assert abs(rec["populations"].sum() - 1.0) < 1e-12 and abs(rec["x"] - state[0].mean()) < 1e-12
    with pytest.raises(ValueError):
        hopping.unpack(np.zeros(11), 3, 40)


def test_the_library_exports_and_the_binding_declares_the_hop_entry_points():
    lib = pkg.load_library()  # no HIP call at load time: works without a GPU
    for name in ("hop_sample", "hop_evolve", "hop_observe"):
        assert name in _capi.GPLE_SYMBOLS
        f = getattr(lib, "gple_" + name)
        assert f.argtypes is not None and len(f.argtypes) == len(_capi.SIGNATURES[name][1])
    assert all(hasattr(_capi.Api, m) for m in ("hop_sample", "hop_evolve", "hop_observe"))
    assert _capi.HOP_REVERSE == 0x2000
