"""CPU: the numpy restatement of gple_hop_outgoing / _mf / _sqc (tests/hop_outgoing_numpy.py), which the GPU tests lean on, against the
restatements of the sums it has to agree with, the driver hopping.run(outgoing=...) on the numpy stand-in apis of all four methods, and the
new symbols of the built library.  What pins the feature, and fails without it: the symbol test (on the library, the header and the binding),
test_run_on_the_stand_ins and test_what_run_refuses_before_any_call (on hopping.run's `outgoing`) and
test_outgoing_density_reads_the_accumulator_as_stated (on hopping.outgoing_density).  The others pin the restatement the GPU tests lean on and
need only the files of tests/: the planes against the sums, a slice onto its complement, the synthetic histogram, and that no trajectory of
the GPU cases is set aside.

The ensembles are those of tests/hop_outgoing_cases.py, evolved by the restatements; the test at the end confirms without a GPU that the
restatement alone sets no trajectory of them aside."""
import os
import re

import numpy as np
import pytest

import gaussian_process_liouville_equation_amd as pkg
from gaussian_process_liouville_equation_amd import _capi, hopping
from tests import hop_mf_numpy as HM
from tests import hop_numpy as HN
from tests import hop_outgoing_cases as HC
from tests import hop_outgoing_numpy as HO
from tests import hop_sqc_numpy as HQ
from tests.conftest import ROOT

TWO32 = 4294967296
MASS = HC.MASS
WIDE = (-1000.0, 2000.0 / 63.0, 64)  # a momentum grid nothing is outside of
NAMES = ("hop_outgoing", "hop_outgoing_mf", "hop_outgoing_sqc")
# t = 0, 430, 860 at p0 = 23.3 (p0 / mass 860 = 10): the centre of the packet is at the right bound, some trajectories have left and some still run
RUN = dict(model=hopping.DAC, num_pes=2, ln_energy=-2.0, n_traj=48, seed=4, dt=4.0, x0=-4.0, xmin=-6.0, xmax=6.0, output_time=430.0, max_outputs=3)
METHODS = ("fssh", "ehrenfest", "sqc", "mash")


def test_the_library_exports_and_the_binding_declares_the_three_entry_points():
    lib = pkg.load_library()  # no HIP call at load time: works without a GPU
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gple.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+gple_%s\s*\(" % name, text), name
        assert name in _capi.GPLE_SYMBOLS and list(_capi.SIGNATURES).count(name) == 1
        f = getattr(lib, "gple_" + name)
        assert f.argtypes is not None and len(f.argtypes) == len(_capi.SIGNATURES[name][1])
        assert hasattr(_capi.Api, name)
    sizes = [len(_capi.SIGNATURES[name][1]) for name in NAMES]
    assert sizes[1] == sizes[0] - 1 and sizes[2] == sizes[1] + 2  # no surface; window and gamma
    assert _capi.TIMER_HOP_OUTGOING == 19 and re.search(r"GPLE_TIMER_HOP_OUTGOING\s*=\s*19\b", text)
    assert (_capi.HOP_AXIS_MOMENTUM, _capi.HOP_AXIS_ENERGY) == (0, 1)
    assert re.search(r"GPLE_HOP_AXIS_MOMENTUM\s+0\b", text) and re.search(r"GPLE_HOP_AXIS_ENERGY\s+1\b", text)


def planes_of(acc, N):
    return acc[:-4].reshape(2, N, -1)


def call(name, kind, grid, axis, state=None, **kw):
    c = HC.case_of(name)
    form, window, gamma = HC.KINDS[kind]
    return HO.outgoing(form, c["potential"], HC.ensemble(name, kind) if state is None else state, MASS, grid, axis, window, gamma, **kw)


@pytest.mark.parametrize("name", list(HC.CASES))
@pytest.mark.parametrize("kind", list(HC.KINDS))
def test_the_planes_add_up_to_the_counts_of_the_sums(name, kind):
    """on a grid nothing is outside of, the sum of a plane over its bins is 2^32 times what the observe call counts for that channel: exactly
    for the surface and the window form; for the amplitude form a side's planes hold one rounding of at most half a unit per term"""
    c = HC.case_of(name)
    N, state = c["N"], HC.ensemble(name, kind)
    form, window, gamma = HC.KINDS[kind]
    acc = call(name, kind, WIDE, "momentum")
    planes, tallies = planes_of(acc, N).sum(axis=2), dict(zip(HO.TALLIES, acc[-4:]))
    assert tallies["outside"] == 0 and tallies["running"] == (state[4] == 0).sum() > 0
    if form == "surface":
        counts = HN.observe(c["potential"], state, MASS)[:3 * N].reshape(3, N)
        assert np.array_equal(planes, TWO32 * counts[1:].astype(np.int64)) and tallies["unassigned"] == 0
    elif form == "window":
        sums = HQ.observe(c["potential"], state, MASS, window, gamma)
        counts, none = sums[:3 * N].reshape(3, N), sums[3 * N + 3:3 * N + 6]
        assert np.array_equal(planes, TWO32 * counts[1:].astype(np.int64)) and tallies["unassigned"] == none[1:].sum() > 0
    else:
        sums = HM.observe(c["potential"], state, MASS)
        weights, n_status = sums[:3 * N].reshape(3, N), sums[3 * N:3 * N + 3]
        # the float sum of the weights itself is rounded: 1e-12 a term covers it
        assert (np.abs(planes.sum(axis=1) - TWO32 * weights[1:].sum(axis=1)) <= N * n_status[1:] * (1.0 + TWO32 * 1e-12)).all()
        assert tallies["unassigned"] == 0
    assert tallies["binned"] == (state[4] != 0).sum() - tallies["unassigned"] and (planes > 0).sum() >= 2
    assert (planes_of(acc, N) >= 0).all()


@pytest.mark.parametrize("kind", list(HC.KINDS))
@pytest.mark.parametrize("axis", ["momentum", "energy"])
def test_a_slice_accumulated_onto_its_complement_is_the_whole(kind, axis):
    c = HC.case_of("tsac")
    form, window, gamma = HC.KINDS[kind]
    state = HC.ensemble("tsac", kind)
    grid = HC.momentum_grid(c["p0"]) if axis == "momentum" else HC.energy_grid(form, c["potential"], state, window, gamma)
    whole = call("tsac", kind, grid, axis)
    part = call("tsac", kind, grid, axis, state=tuple(a[:150] for a in state))
    assert not np.array_equal(part, whole)
    assert np.array_equal(call("tsac", kind, grid, axis, state=tuple(a[150:] for a in state), acc=part), whole)
    assert np.array_equal(call("tsac", kind, grid, axis, skip=np.zeros(HC.N_TRAJ, dtype=bool)), whole)


def test_a_synthetic_momentum_histogram_is_a_direct_count():
    """4099 trajectories with statuses 0 ... 2 and a surface each from a generator, momenta on the integers and halves: the bins are counted by
    hand.  A status of 7 and a surface of -1 are skipped, a NaN is outside"""
    rng = np.random.default_rng(11)
    n, N = 4099, 2
    status = rng.integers(0, 3, n).astype(np.int32)
    surface = rng.integers(0, N, n).astype(np.int32)
    p = rng.integers(-6, 14, n) * 0.5
    status[:3], surface[3:6], p[6:9] = 7, -1, np.nan
    b = np.zeros((n, N), dtype=np.complex128)
    b[:, 0] = 1.0
    state = (np.full(n, 7.0), p, b, surface, status)
    grid = (0.0, 1.0, 5)  # the points 0 ... 4: bin j holds [j - 1/2, j + 1/2)
    acc = HO.outgoing("surface", HN.builtin(HN.DAC, N), state, MASS, grid, "momentum")
    valid = (status >= 1) & (status <= 2) & (surface >= 0)
    want = np.zeros((2, N, 5), dtype=np.int64)
    outside = 0
    for i in np.nonzero(valid)[0]:
        j = -1 if np.isnan(p[i]) else int(np.floor(p[i] + 0.5))
        if 0 <= j < 5:
            want[status[i] - 1, surface[i], j] += TWO32
        else:
            outside += 1
    assert np.array_equal(planes_of(acc, N), want) and (want > 0).all()
    assert list(acc[-4:]) == [want.sum() // TWO32, outside, (status == 0).sum(), 0] and outside > 6


@pytest.mark.parametrize("method", METHODS)
def test_run_on_the_stand_ins(method, tmp_path):
    plain_api, api = HO.APIS[method](), HO.APIS[method]()
    plain = hopping.run(plain_api, method=method, **RUN)
    res = hopping.run(api, method=method, out_dir=str(tmp_path), outgoing={"energy": 32, "momentum": 64}, **RUN)
    # outgoing=None: the calls and the keys of the parent (tests/test_hop_methods_host.py pins both literally); with it the same, then the tail
    assert "outgoing" not in plain and set(res) == set(plain) | {"outgoing"}
    n = len(plain_api.calls)
    suffix = {"fssh": "", "ehrenfest": "_mf", "sqc": "_sqc", "mash": ""}[method]
    tail = (1, 1.0 / 3.0) if method == "sqc" else ()
    assert api.calls[:n] == plain_api.calls and not [c for c in plain_api.calls if c[0].startswith(("outgoing", "adiabatic"))]
    assert api.calls[n:] == [("adiabatic",), ("adiabatic",), ("outgoing" + suffix, "momentum", *tail), ("outgoing" + suffix, "energy", *tail)]
    assert list(res["outgoing"]) == ["momentum", "energy"] and res["scattering_line"] == plain["scattering_line"]
    n_norm = res["n_finished_windowed"] if method == "sqc" else 48
    for axis, bins in (("momentum", 64), ("energy", 32)):
        out = res["outgoing"][axis]
        assert set(out) == {"grid", "density", "acc", "tallies"} and set(out["tallies"]) == set(HO.TALLIES)
        assert len(out["grid"]) == 3 and out["grid"][2] == bins and out["density"].shape == (2, 2, bins) and out["density"].dtype == np.float64
        assert out["acc"].shape == (4 * bins + 4,) and out["acc"].dtype == np.int64
        density, tallies = hopping.outgoing_density(out["acc"], 2, bins, n_norm, out["grid"][1])
        assert np.array_equal(density, out["density"]) and dict(zip(HO.TALLIES, tallies)) == out["tallies"]
        # nobody is outside the default grids: density times step over the bins is the scattering line's fractions
        # (but the SQC Hamiltonian holds the zero-point terms of the other levels: its energies spread beyond the packet's)
        assert out["tallies"]["binned"] > 8 and out["tallies"]["running"] > 0
        assert out["tallies"]["outside"] == 0 or (method, axis) == ("sqc", "energy")
        if out["tallies"]["outside"]:
            continue
        # (counts: to the rounding of the division; weights: each term of a plane was rounded to half a unit of 2^-32)
        bound = 1e-13 + (out["tallies"]["binned"] / 2.0 / TWO32 / n_norm if method == "ehrenfest" else 0.0)
        assert np.abs((out["density"] * out["grid"][1]).sum(axis=2) - res["scattered"]).max() <= bound
    # the files: absorbed_p.txt's and spectrum.txt's layouts, "%g"
    rows = np.loadtxt(tmp_path / "outgoing_p.txt")
    assert rows.shape == (4, 64)
    want = res["outgoing"]["momentum"]["density"].reshape(4, 64)
    assert (np.abs(rows - want) <= 5.1e-6 * np.abs(want)).all()
    rows = np.loadtxt(tmp_path / "outgoing_e.txt")
    grid = res["outgoing"]["energy"]["grid"]
    want = np.column_stack([grid[0] + grid[1] * np.arange(32), res["outgoing"]["energy"]["density"].reshape(4, 32).T])
    assert rows.shape == (32, 5) and (np.abs(rows - want) <= 5.1e-6 * np.abs(want)).all()
    assert sorted(os.listdir(tmp_path)) == ["averages.txt", "outgoing_e.txt", "outgoing_p.txt", "t.txt"]
    # the default grids: the p axis of phase_grid_of, and p0 -+ 3 sigma_p on the start surface
    s = res["setup"]
    assert res["outgoing"]["momentum"]["grid"] == hopping.phase_grid_of(HO.APIS[method](), 2, hopping.DAC, s, (257, 64))[3:]
    E0 = HN.states(np.array([s["x0"]]), HN.builtin(HN.DAC, 2))[1][0, 0]
    low, high = ((s["p0"] + k * s["sigma_p"]) ** 2 / 2.0 / s["mass"] + E0 for k in (-3.0, 3.0))
    assert np.allclose([grid[0], grid[0] + 31 * grid[1]], [low, high], rtol=1e-14, atol=0)
    # a given triple is taken as it is, and one axis alone makes one call
    one = HO.APIS[method]()
    only = hopping.run(one, method=method, outgoing={"energy": (0.0, 0.01, 7)}, **RUN)
    assert list(only["outgoing"]) == ["energy"] and only["outgoing"]["energy"]["grid"] == (0.0, 0.01, 7)
    assert one.calls[n:] == [("outgoing" + suffix, "energy", *tail)]


@pytest.mark.parametrize("bad", [{}, [], 64, {"p": 64}, {"momentum": 64, "x": 3}, {"momentum": 1}, {"momentum": 0}, {"energy": -4}, {"energy": 2.5},
                                 {"energy": True}, {"momentum": (0.0, 1.0)}, {"momentum": (0.0, 0.0, 4)}, {"momentum": (0.0, -1.0, 4)},
                                 {"momentum": (float("nan"), 1.0, 4)}, {"energy": (0.0, float("inf"), 4)}, {"energy": (0.0, 1.0, 0)},
                                 {"energy": (0.0, 1.0, 2.5)}, {"energy": "wide"}])
def test_what_run_refuses_before_any_call(bad):
    api = HO.NumpyOutgoingApi()
    with pytest.raises(ValueError):
        hopping.run(api, outgoing=bad, **RUN)
    assert api.calls == []


def test_outgoing_density_reads_the_accumulator_as_stated():
    acc = np.arange(2 * 3 * 5 + 4, dtype=np.int64) * 1234567891
    density, tallies = hopping.outgoing_density(acc, 3, 5, 7, 0.25)
    w = np.float64(7) * np.float64(0.25)
    assert np.array_equal(density, acc[:30].reshape(2, 3, 5).astype(np.float64) * (1.0 / TWO32) / w) and tallies == tuple(int(v) for v in acc[30:])
    for bad in (lambda: hopping.outgoing_density(acc[:-1], 3, 5, 7, 0.25), lambda: hopping.outgoing_density(acc, 3, 5, 0, 0.25)):
        with pytest.raises(ValueError):
            bad()


@pytest.mark.parametrize("name", list(HC.CASES))
@pytest.mark.parametrize("kind", list(HC.KINDS))
def test_the_restatement_alone_sets_no_trajectory_of_the_gpu_cases_aside(name, kind):
    """what tests/test_gpu_hop_outgoing.py may set aside, formed on the restatement's own ensembles: seed 0 gives none, on either axis"""
    assert np.finfo(np.longdouble).eps < 1e-18  # or the margins calibrate nothing
    c = HC.case_of(name)
    form, window, gamma = HC.KINDS[kind]
    state = HC.ensemble(name, kind)
    for axis, grid in (("momentum", HC.momentum_grid(c["p0"])), ("energy", HC.energy_grid(form, c["potential"], state, window, gamma))):
        aside, m = HC.set_aside(form, c["potential"], state, grid, axis, window, gamma)
        assert not aside.any(), (axis, m["edge"].min(), m["window"].min())
        acc = HO.outgoing(form, c["potential"], state, MASS, grid, axis, window, gamma)
        assert acc[-4] > 0 and acc[-2] > 0 and (planes_of(acc, c["N"]).sum(axis=2) > 0).sum() >= 2
        assert axis == "momentum" or acc[-3] == 0  # the energy grid is made around the finished trajectories
        assert m["D_w"].max() <= 1e-13
