"""CPU: the numpy restatement of the grouped surface hopping calls (tests/hop_scan_numpy.py), which the GPU tests lean on, the driver hopping.scan
on a numpy stand-in api against per-group loops over the plain calls, and the new symbols of the built library (the one test here that fails
without the feature)."""
import re
from pathlib import Path

import numpy as np
import pytest

import gaussian_process_liouville_equation_amd as pkg
from gaussian_process_liouville_equation_amd import _capi, exact, hopping
from tests import hop_numpy as HN
from tests import hop_scan_numpy as HS

MASS, X0, LEFT, RIGHT = 2000.0, -4.0, -6.0, 6.0
P0 = (8.0, 10.0, 16.0, 24.0, 30.0)
DT = (2.0, 2.0, 1.0, 1.0, 0.5)


def packets_of(p0s, sigma=True):
    return np.array([[X0, p0, 1.0 / (2.0 * p0 / 20.0) if sigma else 0.0, p0 / 20.0 if sigma else 0.0] for p0 in p0s])


def same_bits(a, b):
    return all(np.array_equal(u, v) and u.dtype == v.dtype for u, v in zip(a, b))


def test_groups_are_the_plain_calls_on_slices():
    pot = HN.builtin(HN.DAC, 2)
    n_per, offset, seed = 7, 1000, 3
    packets = packets_of(P0)
    state = HS.sample_groups(pot, 2, n_per, seed, packets, trajectory_offset=offset)
    end, hops, diag = HS.evolve_groups(pot, state, n_per, seed, MASS, DT, 0, 120, LEFT, RIGHT, trajectory_offset=offset)
    rows = HS.observe_groups(pot, end, n_per, MASS)
    assert rows.shape == (5, 11)
    for g, sl in enumerate(HS.slices(5, n_per)):
        part = HN.sample(pot, 2, n_per, seed, *packets[g], trajectory_offset=offset + g * n_per)
        assert same_bits(part, tuple(a[sl] for a in state))
        part, d = HN.evolve(pot, part, seed, MASS, DT[g], 0, 120, LEFT, RIGHT, trajectory_offset=offset + g * n_per)
        assert same_bits(part, tuple(a[sl] for a in end))
        assert np.array_equal(hops[sl, 0], d["hops"]) and np.array_equal(hops[sl, 1], d["frustrated"])
        assert np.array_equal(rows[g], HN.observe(pot, part, MASS))
    # equal packets and equal time steps: the plain call over the whole
    same = np.repeat(packets[2:3], 3, axis=0)
    state = HS.sample_groups(pot, 2, n_per, seed, same, trajectory_offset=offset)
    whole = HN.sample(pot, 2, 3 * n_per, seed, *same[0], trajectory_offset=offset)
    assert same_bits(state, whole)
    end, _, _ = HS.evolve_groups(pot, state, n_per, seed, MASS, [1.0] * 3, 0, 120, LEFT, RIGHT, trajectory_offset=offset)
    assert same_bits(end, HN.evolve(pot, whole, seed, MASS, 1.0, 0, 120, LEFT, RIGHT, trajectory_offset=offset)[0])


@pytest.mark.parametrize("model,N,surface0", [(HN.DAC, 2, 0), (HN.TSAC, 3, 1)])
def test_zero_sigmas_give_the_centre_exactly(model, N, surface0):
    pot = HN.builtin(model, N)
    packets = np.array([[X0, 10.0, 0.0, 0.0], [-3.5, 16.0, 0.0, 0.8], [-0.0, 12.0, 0.3, 0.0]])
    x, p, b, surface, status = HS.sample_groups(pot, N, 9, 5, packets, surface0)
    for g, sl in enumerate(HS.slices(3, 9)):
        x0, p0, sx, sp = packets[g]
        if sx == 0.0:
            assert np.array_equal(x[sl], np.full(9, x0)) and np.array_equal(np.signbit(x[sl]), np.full(9, np.signbit(x0)))
        else:
            assert len(np.unique(x[sl])) == 9
        if sp == 0.0:
            assert np.array_equal(p[sl], np.full(9, p0))
        else:
            assert len(np.unique(p[sl])) == 9
    _, _, C, _ = HN.states(x, pot)
    assert np.array_equal(b, C[:, :, surface0].astype(np.complex128))  # the column of C(x0) where x is x0
    assert (surface == surface0).all() and (status == 0).all()
    assert np.array_equal(b[:9], np.repeat(b[:1], 9, axis=0))


def test_the_counters_are_the_hops_of_single_steps():
    pot, reverse = HN.builtin(HN.DAC, 2), True
    n_per, seed, steps = 40, 2, 900
    p0s, dts = (8.0, 10.0), (2.0, 1.0)
    state = HS.sample_groups(pot, 2, n_per, seed, packets_of(p0s))
    end, hops, diag = HS.evolve_groups(pot, state, n_per, seed, MASS, dts, 0, steps, LEFT, RIGHT, reverse)
    walk, taken, counted = state, np.zeros(2 * n_per, dtype=np.int64), None
    for s in range(steps):
        nxt, counted, _ = HS.evolve_groups(pot, walk, n_per, seed, MASS, dts, s, 1, LEFT, RIGHT, reverse, hops=counted)
        taken += nxt[3] != walk[3]
        walk = nxt
    assert same_bits(walk, end) and np.array_equal(counted, hops) and counted.dtype == np.int32
    assert np.array_equal(hops[:, 0], taken) and np.array_equal(hops[:, 1], diag["frustrated"])
    assert hops[:, 0].sum() >= 5 and hops[:, 1].sum() >= 2  # at these momenta some hops are frustrated
    # added to what is there, and a null counter changes no state
    again, more, _ = HS.evolve_groups(pot, state, n_per, seed, MASS, dts, 0, steps, LEFT, RIGHT, reverse, hops=hops)
    assert np.array_equal(more, 2 * hops) and same_bits(again, end)


SCAN = dict(model=hopping.DAC, num_pes=2, momenta=[10.0, 16.0, 30.0], n_per_group=16, seed=1, dt=[4.0, 2.0, 2.0], x0=X0, xmin=LEFT, xmax=RIGHT)


def loop_over_groups(api, res, fixed):
    """what a user writes without the grouped calls: per momentum one sample, one evolve of the scan's steps and one observe, with the offset"""
    rows = []
    for g, s in enumerate(res["setups"]):
        off = g * res["n_per_group"]
        sx, sp = (0.0, 0.0) if fixed else (s["sigma_x"], s["sigma_p"])
        st = api.hop_sample(2, hopping.DAC, res["n_per_group"], SCAN["seed"], s["x0"], s["p0"], sx, sp, 0, trajectory_offset=off)
        st = api.hop_evolve(2, hopping.DAC, st, SCAN["seed"], s["mass"], res["dt"][g], 0, res["steps"], s["xmin"], s["xmax"], trajectory_offset=off)
        rows.append(api.hop_observe(2, hopping.DAC, st, s["mass"]))
    return np.array(rows)


@pytest.mark.parametrize("fixed", [True, False])
def test_scan_until_nobody_runs(tmp_path, fixed):
    api = HS.NumpyScanApi()
    res = hopping.scan(api, fixed=fixed, chunk_steps=128, out_dir=str(tmp_path), **SCAN)
    assert res["stop"] is not None and "NO TRAJECTORY IS RUNNING" in res["stop"]
    assert res["steps"] % 128 == 0 and 0 < res["steps"] <= res["max_steps"] == max(res["total_step"])
    assert res["total_step"] == [int(s["total_time"] / t) for s, t in zip(res["setups"], SCAN["dt"])]
    # one sample, an observe, then an evolve of chunk_steps steps and an observe per launch
    calls = api.calls
    assert calls[0] == ("sample_groups", 3, 16) and calls[1] == ("observe_groups",)
    assert calls[2::2] == [("evolve_groups", k * 128, 128) for k in range(res["steps"] // 128)] and all(c == ("observe_groups",) for c in calls[3::2])
    rows = loop_over_groups(HN.NumpyHopApi(), res, fixed)
    assert np.array_equal(res["rows"], rows)
    counts = rows[:, :6].reshape(3, 3, 2)
    assert np.array_equal(res["scattered"], counts[:, 1:] / 16) and not res["running"].any() and (counts.sum(axis=(1, 2)) == 16).all()
    # scan.txt: head, 4 fractions, running, their 5 standard errors, hops, frustrated, drift
    lines = [[float(v) for v in line.split()] for line in open(tmp_path / "scan.txt")]
    assert len(lines) == 3 and all(len(line) == 1 + 5 + 5 + 3 for line in lines)
    for g, line in enumerate(lines):
        s = res["setups"][g]
        f = np.array([*res["scattered"][g].reshape(-1), res["running"][g]])
        want = [np.log(s["p0"] ** 2 / 2.0 / s["mass"]), *f, *np.sqrt(f * (1.0 - f) / 16), res["hops"][g], res["frustrated"][g], res["energy_drift"][g]]
        assert np.allclose(line, want, rtol=1e-5, atol=1e-300)
        assert np.array_equal(res["stderr"][g], np.sqrt(f * (1.0 - f) / 16)) and abs(f.sum() - 1.0) < 1e-12
        assert exact.fmt(want[0]) == res["lines"][g].split()[0] and res["head"][g] == want[0]
    per = np.asarray(res["hop_counts"]).reshape(3, 16, 2).sum(axis=1) / 16
    assert np.array_equal(res["hops"], per[:, 0]) and np.array_equal(res["frustrated"], per[:, 1]) and res["hops"].sum() > 0
    first = HS.observe_groups(HN.builtin(HN.DAC, 2), HS.sample_groups(HN.builtin(HN.DAC, 2), 2, 16, SCAN["seed"], [[s["x0"], s["p0"], 0.0 if fixed else s["sigma_x"],
                              0.0 if fixed else s["sigma_p"]] for s in res["setups"]]), 16, MASS)
    assert np.array_equal(res["energy_drift"], (rows[:, -1] - first[:, -1]) / 16) and np.abs(res["energy_drift"]).max() < 1e-3


def test_scan_stops_at_max_steps_and_does_not_depend_on_the_chunk():
    res = hopping.scan(HS.NumpyScanApi(), fixed=False, chunk_steps=64, max_steps=200, **SCAN)
    assert res["stop"] is None and res["steps"] == 200 and res["running"].sum() > 0
    assert np.array_equal(res["rows"], loop_over_groups(HN.NumpyHopApi(), res, False))
    api = HS.NumpyScanApi()
    other = hopping.scan(api, fixed=False, chunk_steps=77, max_steps=200, **SCAN)
    assert [c for c in api.calls if c[0] == "evolve_groups"] == [("evolve_groups", 0, 77), ("evolve_groups", 77, 77), ("evolve_groups", 154, 46)]
    assert same_bits(res["state"], other["state"]) and np.array_equal(res["hop_counts"], other["hop_counts"]) and res["lines"] == other["lines"]
    # the default time step is the setup's rule, per group; ln_energies name the same groups as their momenta
    s = exact.setup(-2.0, boundary=exact.ABSORBING, x0=X0, xmin=LEFT, xmax=RIGHT)
    short = hopping.scan(HS.NumpyScanApi(), ln_energies=[-2.0, -1.0], n_per_group=2, max_steps=3, x0=X0, xmin=LEFT, xmax=RIGHT)
    assert short["dt"][0] == s["dt_rule"] and short["steps"] == 3 and short["setups"][0]["p0"] == s["p0"]
    assert abs(short["head"][0] + 2.0) < 1e-12 and abs(short["head"][1] + 1.0) < 1e-12
    # Tully's convention is the default: before the first step every trajectory of a point sits at x0 with exactly p0
    start = hopping.scan(HS.NumpyScanApi(), ln_energies=[-2.0, -1.0], n_per_group=2, max_steps=0, x0=X0, xmin=LEFT, xmax=RIGHT)
    assert start["steps"] == 0 and start["stop"] is None and (start["running"] == 1.0).all() and not start["energy_drift"].any()
    assert (start["state"][0] == X0).all() and np.array_equal(start["state"][1], np.repeat([t["p0"] for t in start["setups"]], 2))


def test_scan_refuses_what_the_groups_cannot_share():
    kw = dict(SCAN, n_per_group=2, max_steps=0)
    for bad in (dict(mass=[2000.0, 2000.0, 1000.0]), dict(xmin=[-6.0, -6.0, -7.0]), dict(xmax=[6.0, 8.0, 6.0])):
        with pytest.raises(ValueError):
            hopping.scan(HS.NumpyScanApi(), **{**kw, **bad})
    with pytest.raises(ValueError):
        hopping.scan(HS.NumpyScanApi(), **{**kw, "x0": [-4.0, -4.0]})  # two values for three groups
    with pytest.raises(ValueError):
        hopping.scan(HS.NumpyScanApi(), ln_energies=[0.0], **kw)  # both
    with pytest.raises(ValueError):
        hopping.scan(HS.NumpyScanApi(), n_per_group=2)  # neither
    ok = hopping.scan(HS.NumpyScanApi(), **{**kw, "x0": [-4.0, -4.5, -5.0], "mass": [2000.0] * 3})  # a value per group that may differ
    assert np.array_equal(ok["state"][0], np.repeat([-4.0, -4.5, -5.0], 2))


def test_the_library_exports_and_the_binding_declares_the_grouped_entry_points():
    lib = pkg.load_library()  # no HIP call at load time: works without a GPU
    for name in ("hop_sample_groups", "hop_evolve_groups", "hop_observe_groups"):
        assert name in _capi.GPLE_SYMBOLS
        f = getattr(lib, "gple_" + name)
        assert f.argtypes is not None and len(f.argtypes) == len(_capi.SIGNATURES[name][1])
        assert hasattr(_capi.Api, name)
    text = (Path(__file__).resolve().parent.parent / "include" / "gple.h").read_text()
    for name in ("gple_hop_sample_groups", "gple_hop_evolve_groups", "gple_hop_observe_groups"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text)
    assert re.search(r"GPLE_TIMER_HOP_GROUPS\s*=\s*14\b", text) and _capi.TIMER_HOP_GROUPS == 14
    assert re.search(r"GPLE_HOP_MAX_GROUPS\s+65536ul", text) and _capi.HOP_MAX_GROUPS == 65536
    assert callable(hopping.scan)
