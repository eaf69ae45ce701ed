"""CPU: the numpy restatement of the surface hopping step with the decoherence correction 6a (tests/hop_deco_numpy.py), which the GPU tests of
tests/test_gpu_hop_deco.py lean on; hopping.run and hopping.scan with the keywords decoherence and edc_c on stand-in apis; and the new symbols
of the built library (the one test here that fails without the feature)."""
import re
from pathlib import Path

import numpy as np
import pytest

import gaussian_process_liouville_equation_amd as pkg
from gaussian_process_liouville_equation_amd import _capi, hopping
from tests import hop_deco_numpy as HD
from tests import hop_numpy as HN
from tests import hop_scan_numpy as HS

MASS, LEFT, RIGHT, X0 = 2000.0, -6.0, 6.0, -4.0
EPS = np.finfo(np.float64).eps
ACTIVE = (HD.EDC, HD.COLLAPSE_HOP, HD.COLLAPSE_ATTEMPT)
ALL = (HD.NONE,) + ACTIVE


def ensemble(potential, num_pes, n, p0, seed=11, surface0=0, dtype=np.float64):
    return HN.sample(potential, num_pes, n, seed, X0, p0, 1.0 / (2.0 * p0 / 20.0), p0 / 20.0, surface0=surface0, dtype=dtype)


def same_bits(a, b):
    return all(np.array_equal(u, v) and u.dtype == v.dtype for u, v in zip(a, b))


def widen(state):
    x, p, b, surface, status = state
    return x.astype(np.longdouble), p.astype(np.longdouble), b.astype(np.clongdouble), surface, status


# ---- mode NONE is the step of hop_numpy ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,N,p0,dt,steps,surface0,reverse", [(HN.DAC, 2, 10.0, 2.0, 500, 0, True), (HN.TSAC, 3, 10.0, 4.0, 200, 1, False)])
def test_mode_none_has_the_bits_of_the_plain_restatement(model, N, p0, dt, steps, surface0, reverse):
    pot = HN.builtin(model, N)
    state = ensemble(pot, N, 24, p0, surface0=surface0)
    want, dw = HN.evolve(pot, state, 5, MASS, dt, 3, steps, LEFT, RIGHT, reverse, 7)
    for decoherence in (None, "none", HD.NONE):
        got, dg = HD.evolve(pot, state, 5, MASS, dt, 3, steps, LEFT, RIGHT, reverse, 7, decoherence=decoherence)
        assert same_bits(got, want) and all(np.array_equal(dg[k], dw[k]) for k in dw)
    assert dw["hops"].sum() >= 5
    wide, _ = HD.evolve(pot, widen(state), 5, MASS, dt, 3, steps, LEFT, RIGHT, reverse, 7)
    assert same_bits(wide, HN.evolve(pot, widen(state), 5, MASS, dt, 3, steps, LEFT, RIGHT, reverse, 7)[0]) and wide[0].dtype == np.longdouble


# ---- the stage alone ----------------------------------------------------------------------------------------------------------------------------
def random_amplitudes(m, N, seed):
    rng = np.random.default_rng(seed)
    c = rng.normal(size=(m, N)) + 1j * rng.normal(size=(m, N))
    c *= rng.uniform(0.5, 1.0, m)[:, None] / np.sqrt(np.sum(np.abs(c) ** 2, axis=1))[:, None]  # 6a keeps the norm the vector has, whatever it is
    E = np.sort(rng.uniform(-0.1, 0.1, (m, N)), axis=1)
    return c, E, rng.integers(0, N, m), rng.uniform(-30.0, 30.0, m)


@pytest.mark.parametrize("N", [2, 3])
def test_edc_damps_the_others_and_keeps_the_norm(N):
    m, dt, edc_c = 256, 2.0, 0.1
    c, E, a, p = random_amplitudes(m, N, N)
    out, changed = HD.stage(c, E, a, p, MASS, dt, HD.EDC, edc_c)
    assert changed.all()
    kinetic = p * p / 2.0 / MASS
    w = kinetic / (kinetic + edc_c)
    row = np.arange(m)
    for k in range(N):
        f = np.exp(-dt * np.abs(E[:, k] - E[row, a]) * w)
        other = a != k
        before, after = np.abs(c[:, k]) ** 2, np.abs(out[:, k]) ** 2
        assert np.abs(after - f * f * before)[other].max() <= 4 * EPS
        assert np.array_equal(np.angle(out[other, k]), np.angle(c[other, k])) or np.abs(np.angle(out[other, k]) - np.angle(c[other, k])).max() <= 4 * EPS
    norm0, norm1 = np.sum(np.abs(c) ** 2, axis=1), np.sum(np.abs(out) ** 2, axis=1)
    assert np.abs(norm1 - norm0).max() <= 4 * EPS * norm0.max()
    assert np.abs(np.angle(out[row, a]) - np.angle(c[row, a])).max() <= 4 * EPS and (np.abs(out[row, a]) >= np.abs(c[row, a])).all()
    # edc_c = 0: w = 1, whatever the momentum is (p = 0 included)
    p[:8] = 0.0
    free, _ = HD.stage(c, E, a, p, MASS, dt, HD.EDC, 0.0)
    for k in range(N):
        f = np.exp(-dt * np.abs(E[:, k] - E[row, a]))
        assert np.abs(np.abs(free[:, k]) ** 2 - f * f * np.abs(c[:, k]) ** 2)[a != k].max() <= 4 * EPS
    assert np.isfinite(free.real).all() and np.abs(np.sum(np.abs(free) ** 2, axis=1) - norm0).max() <= 4 * EPS * norm0.max()
    # a larger constant damps less
    weak, _ = HD.stage(c, E, a, p, MASS, dt, HD.EDC, 10.0)
    k0 = (a + 1) % N
    assert (np.abs(weak[row, k0])[8:] > np.abs(out[row, k0])[8:]).all()


@pytest.mark.parametrize("N", [2, 3])
def test_a_collapse_leaves_a_unit_amplitude_with_its_phase(N):
    m = 256
    c, E, a, p = random_amplitudes(m, N, 10 + N)
    rng = np.random.default_rng(1)
    wanted = rng.random(m) < 0.5
    taken = wanted & (rng.random(m) < 0.5)
    row = np.arange(m)
    for mode, which in ((HD.COLLAPSE_HOP, taken), (HD.COLLAPSE_ATTEMPT, wanted)):
        out, changed = HD.stage(c, E, a, p, MASS, 2.0, mode, 0.1, wanted=wanted, taken=taken)
        assert np.array_equal(changed, which) and which.any() and (~which).any()
        assert np.array_equal(out[~which], c[~which])
        hit = out[which]
        ah = a[which]
        others = np.arange(N)[None, :] != ah[:, None]
        assert np.all(hit[others] == 0.0)
        ca = hit[np.arange(len(ah)), ah]
        assert np.abs(np.abs(ca) - 1.0).max() <= 4 * EPS
        assert np.abs(np.angle(ca) - np.angle(c[which][np.arange(len(ah)), ah])).max() <= 4 * EPS
        assert same_bits(HD.stage(c, E, a, p, MASS, 2.0, mode, 7.0, wanted=wanted, taken=taken), (out, changed))  # edc_c is not read


def test_a_zero_active_amplitude_skips_the_stage():
    m, N = 32, 3
    c, E, a, p = random_amplitudes(m, N, 3)
    c[np.arange(m), a] = 0.0
    yes = np.ones(m, dtype=bool)
    for mode in ALL:
        out, changed = HD.stage(c, E, a, p, MASS, 2.0, mode, 0.1, wanted=yes, taken=yes)
        assert not changed.any() and np.array_equal(out, c)
    out, changed = HD.stage(c, E, a, p, MASS, 2.0, HD.NONE)
    assert not changed.any() and np.array_equal(out, c)
    with pytest.raises((ValueError, KeyError)):
        HD.mode_of(4)


# ---- the whole step -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ALL)
def test_the_amplitudes_stay_normalised(mode):
    """|sum |b|^2 - 1| <= 1e-12 over 1000 steps: EDC and b <- C c keep the norm to rounding, a collapse restores it"""
    pot = HN.builtin(HN.DAC, 2)
    state = ensemble(pot, 2, 64, 16.0)
    (x, p, b, surface, status), diag = HD.evolve(pot, state, 11, MASS, 1.0, 0, 1000, -1e3, 1e3, decoherence=mode)
    worst = np.abs(np.sum(np.abs(b) ** 2, axis=1) - 1.0).max()
    print(f"hop deco norm, mode {mode}: hops {diag['hops'].sum()}, | |b|^2 - 1 | {worst:.3g}")
    assert (status == 0).all() and diag["hops"].sum() >= 10
    assert worst <= 1e-12


@pytest.mark.parametrize("mode", ACTIVE)
def test_the_correction_changes_the_run(mode):
    pot = HN.builtin(HN.DAC, 2)
    state = ensemble(pot, 2, 96, 10.0)
    plain, _ = HN.evolve(pot, state, 11, MASS, 2.0, 0, 900, LEFT, RIGHT)
    got, diag = HD.evolve(pot, state, 11, MASS, 2.0, 0, 900, LEFT, RIGHT, decoherence=mode)
    assert diag["hops"].sum() >= 10 and not np.array_equal(got[2], plain[2])
    if mode == HD.EDC:  # and its constant matters
        assert not np.array_equal(HD.evolve(pot, state, 11, MASS, 2.0, 0, 900, LEFT, RIGHT, decoherence=mode, edc_c=1.0)[0][2], got[2])
        # far from the coupling region the amplitudes of a damped run sit on the active surface
        x, _, b, surface, status = got
        _, _, C, _ = HN.states(x, pot)
        c = np.einsum("mik,mi->mk", C, b)
        assert np.mean(np.abs(c[np.arange(96), surface]) ** 2) > 0.99


@pytest.mark.parametrize("model,N,p0,dt,steps,surface0", [(HN.DAC, 2, 10.0, 2.0, 600, 0), (HN.TSAC, 3, 10.0, 4.0, 200, 1)])
@pytest.mark.parametrize("mode", ALL)
def test_the_sign_of_the_eigenvectors_changes_nothing(mode, model, N, p0, dt, steps, surface0):
    pot = HN.builtin(model, N)
    state = ensemble(pot, N, 96, p0, surface0=surface0)
    plain, d0 = HD.evolve(pot, state, 11, MASS, dt, 0, steps, LEFT, RIGHT, decoherence=mode)
    flipped, d1 = HD.evolve(pot, state, 11, MASS, dt, 0, steps, LEFT, RIGHT, flip=True, decoherence=mode)
    wide, _ = HD.evolve(pot, widen(state), 11, MASS, dt, 0, steps, LEFT, RIGHT, decoherence=mode)
    assert d0["hops"].sum() >= 10
    assert np.array_equal(d0["hops"], d1["hops"]) and np.array_equal(d0["frustrated"], d1["frustrated"])
    assert np.array_equal(plain[3], flipped[3]) and np.array_equal(plain[4], flipped[4])
    for q in range(3):  # x, p, and the diabatic amplitudes do not see the flip either: within the D floor
        D = np.abs(plain[q] - wide[q]).max()
        assert np.abs(plain[q] - flipped[q]).max() <= HN.tolerance(D, plain[q]), (q, D)


@pytest.mark.parametrize("mode", ALL)
def test_evolve_carries_nothing_hidden(mode):
    pot = HN.builtin(HN.DAC, 2)
    state = ensemble(pot, 2, 48, 10.0)
    args = dict(decoherence=mode, edc_c=0.1)
    whole, _ = HD.evolve(pot, state, 3, MASS, 2.0, 0, 400, LEFT, RIGHT, **args)
    half, _ = HD.evolve(pot, state, 3, MASS, 2.0, 0, 150, LEFT, RIGHT, **args)
    rest, _ = HD.evolve(pot, half, 3, MASS, 2.0, 150, 250, LEFT, RIGHT, **args)
    assert same_bits(whole, rest)
    part, _ = HD.evolve(pot, tuple(a[20:] for a in state), 3, MASS, 2.0, 0, 400, LEFT, RIGHT, trajectory_offset=20, **args)
    assert same_bits(tuple(a[20:] for a in whole), part)


@pytest.mark.parametrize("mode", ALL)
def test_groups_are_the_plain_restatement_on_slices(mode):
    pot = HN.builtin(HN.DAC, 2)
    n_per, seed, steps, offset = 9, 2, 500, 50
    p0s, dts = np.array([8.0, 10.0, 16.0, 24.0]), np.array([2.0, 2.0, 1.0, 1.0])
    packets = np.stack([np.full(4, X0), p0s, 1.0 / (2.0 * p0s / 20.0), p0s / 20.0], axis=1)
    state = HS.sample_groups(pot, 2, n_per, seed, packets, 0, offset)
    before = np.full((4 * n_per, 2), 3, dtype=np.int32)
    end, hops, diag = HD.evolve_groups(pot, state, n_per, seed, MASS, dts, 0, steps, LEFT, RIGHT, True, offset, hops=before, decoherence=mode)
    assert (before == 3).all() and hops.dtype == np.int32
    for g, sl in enumerate(HS.slices(4, n_per)):
        part, d = HD.evolve(pot, tuple(a[sl] for a in state), seed, MASS, dts[g], 0, steps, LEFT, RIGHT, True, offset + g * n_per, decoherence=mode)
        assert same_bits(part, tuple(a[sl] for a in end)), g
        assert np.array_equal(hops[sl, 0], 3 + d["hops"]) and np.array_equal(hops[sl, 1], 3 + d["frustrated"])
        assert np.array_equal(diag["margin"][sl], d["margin"])
    assert hops[:, 0].sum() - 3 * 4 * n_per >= 5
    if mode == HD.NONE:
        want, counted, _ = HS.evolve_groups(pot, state, n_per, seed, MASS, dts, 0, steps, LEFT, RIGHT, True, offset, hops=before)
        assert same_bits(end, want) and np.array_equal(hops, counted)


# ---- the drivers --------------------------------------------------------------------------------------------------------------------------------
RUN = dict(model=hopping.DAC, num_pes=2, ln_energy=-2.0, n_traj=32, seed=4, dt=4.0, x0=X0, xmin=LEFT, xmax=RIGHT)
SCAN = dict(model=hopping.DAC, num_pes=2, momenta=[10.0, 16.0], n_per_group=12, seed=1, dt=[4.0, 2.0], chunk_steps=128, x0=X0, xmin=LEFT, xmax=RIGHT)


def files_of(directory):
    return {path.name: path.read_bytes() for path in sorted(Path(directory).iterdir())}


def test_run_without_a_correction_calls_the_api_as_before(tmp_path):
    old, new = HN.NumpyHopApi(), HD.NumpyDecoApi()  # the first does not know the keywords: passing one raises TypeError
    a = hopping.run(old, out_dir=str(tmp_path / "a"), **RUN)
    b = hopping.run(new, out_dir=str(tmp_path / "b"), decoherence=None, **RUN)
    assert old.calls == new.calls and len(new.keywords) == len(a["records"]) - 1 > 3
    assert all(k == (None, HD.EDC_C) for k in new.keywords)  # the stand-in's own defaults: nothing was passed
    assert same_bits(a["state"], b["state"]) and a["scattering_line"] == b["scattering_line"]
    assert files_of(tmp_path / "a") == files_of(tmp_path / "b") and sorted(files_of(tmp_path / "a")) == ["averages.txt", "t.txt"]
    assert a["decoherence"] is None and a["edc_c"] == 0.1 and b["decoherence"] is None


def test_run_forwards_the_correction_to_every_evolve(tmp_path):
    api = HD.NumpyDecoApi()
    res = hopping.run(api, out_dir=str(tmp_path), decoherence="edc", edc_c=0.25, **RUN)
    assert len(api.keywords) == len(res["records"]) - 1 > 3 and all(k == ("edc", 0.25) for k in api.keywords)
    assert res["decoherence"] == "edc" and res["edc_c"] == 0.25 and res["stop"] is not None
    # the same loop by hand
    s = res["setup"]
    pot = HN.builtin(HN.DAC, 2)
    state = HN.sample(pot, 2, 32, 4, s["x0"], s["p0"], s["sigma_x"], s["sigma_p"])
    state, _ = HD.evolve(pot, state, 4, s["mass"], 4.0, 0, res["steps"], LEFT, RIGHT, decoherence=HD.EDC, edc_c=0.25)
    assert same_bits(state, res["state"])
    plain = hopping.run(HN.NumpyHopApi(), **RUN)
    assert not np.array_equal(plain["state"][2], res["state"][2])
    # averages.txt keeps its layout; the mean |c_k|^2 now follows the fraction on surface k once everybody is far out
    last = [float(v) for v in open(tmp_path / "averages.txt").read().splitlines()[-1].split()]
    assert len(last) == 4 + 2 * 2 and np.abs(np.array(last[4:6]) - np.array(last[6:8])).max() < 0.02
    with pytest.raises(TypeError):
        hopping.run(HN.NumpyHopApi(), decoherence="edc", **RUN)  # an api without the feature says so, nothing is dropped silently


def test_scan_without_a_correction_calls_the_api_as_before(tmp_path):
    old, new = HS.NumpyScanApi(), HD.NumpyDecoApi()
    a = hopping.scan(old, out_dir=str(tmp_path / "a"), **SCAN)
    b = hopping.scan(new, out_dir=str(tmp_path / "b"), decoherence=None, **SCAN)
    assert old.calls == new.calls and len(new.keywords) == -(-a["steps"] // 128) > 1 and all(k == (None, HD.EDC_C) for k in new.keywords)
    assert same_bits(a["state"], b["state"]) and np.array_equal(a["hop_counts"], b["hop_counts"]) and a["lines"] == b["lines"]
    assert files_of(tmp_path / "a") == files_of(tmp_path / "b") and list(files_of(tmp_path / "a")) == ["scan.txt"]
    assert a["decoherence"] is None and a["edc_c"] == 0.1


def test_scan_forwards_the_correction_to_every_evolve():
    api = HD.NumpyDecoApi()
    res = hopping.scan(api, decoherence="edc", edc_c=0.05, **SCAN)
    assert len(api.keywords) == -(-res["steps"] // 128) > 1 and all(k == ("edc", 0.05) for k in api.keywords)
    assert res["decoherence"] == "edc" and res["edc_c"] == 0.05
    pot = HN.builtin(HN.DAC, 2)
    packets = [[s["x0"], s["p0"], 0.0, 0.0] for s in res["setups"]]
    state = HS.sample_groups(pot, 2, 12, 1, packets)
    state, hops, _ = HD.evolve_groups(pot, state, 12, 1, MASS, res["dt"], 0, res["steps"], LEFT, RIGHT, decoherence=HD.EDC, edc_c=0.05)
    assert same_bits(state, res["state"]) and np.array_equal(hops, res["hop_counts"])
    assert all(len(line.split()) == 14 for line in res["lines"])
    with pytest.raises(TypeError):
        hopping.scan(HS.NumpyScanApi(), decoherence="collapse_hop", **SCAN)


# ---- the symbols (fails without the feature; no GPU) ----------------------------------------------------------------------------------------------
def test_the_library_exports_and_the_binding_declares_the_decoherence_entry_points():
    lib = pkg.load_library()  # no HIP call at load time: works without a GPU
    for name, base in (("hop_evolve_dc", "hop_evolve"), ("hop_evolve_groups_dc", "hop_evolve_groups")):
        assert name in _capi.GPLE_SYMBOLS
        f = getattr(lib, "gple_" + name)
        assert f.argtypes is not None and len(f.argtypes) == len(_capi.SIGNATURES[name][1]) == len(_capi.SIGNATURES[base][1]) + 2
    text = (Path(__file__).resolve().parent.parent / "include" / "gple.h").read_text()
    for name in ("gple_hop_evolve_dc", "gple_hop_evolve_groups_dc"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text)
    for k, name in enumerate(("NONE", "EDC", "COLLAPSE_HOP", "COLLAPSE_ATTEMPT")):
        assert re.search(r"#define\s+GPLE_HOP_DC_%s\s+%d\b" % (name, k), text) and getattr(_capi, "HOP_DC_" + name) == k == getattr(HD, name)
    assert _capi.HOP_DC_NAMES == {"none": 0, "edc": 1, "collapse_hop": 2, "collapse_attempt": 3}
    assert _capi.Api._hop_decoherence("collapse_attempt") == 3 and _capi.Api._hop_decoherence(2) == 2
    with pytest.raises(ValueError):
        _capi.Api._hop_decoherence("tully")
