"""GPU: what left the box per channel (gple_hop_outgoing / _mf / _sqc, csrc/gple_hop.hip; DESIGN.md §17 "What left the box") against the numpy
restatement tests/hop_outgoing_numpy.py and against the device's own sums.

Every state is the DEVICE's own ensemble of tests/hop_outgoing_cases.py after its sample and its step calls, read back: the same arrays go to
the device call and to the restatement, so a difference is the binning's alone.  64 bins.  On the momentum axis the bin is four IEEE
operations on the stored p: every word must be EQUAL and nothing is set aside.  On the energy axis q_E is recomputed on either side, so a
trajectory is set aside where its long double q_E lies within 1e-9 step of a cell edge (its weight may then sit in either neighbouring
bin), and with the window form where some e_k is within 1e-10 of a window edge; at most 2 of 293, and seed 0 gives none
(tests/test_hop_outgoing_host.py asserts that on the restatement's own ensembles).  A weight of the amplitude form is a rounded float: a word
lies within the sum over the restatement's trajectories of that word of 2^32 (64 D_w + 1e-13) + 1, D_w the float64 against long double
difference of the weight."""
import ctypes as C

import numpy as np
import pytest

from gaussian_process_liouville_equation_amd import _capi, hopping
from tests import hop_numpy as HN
from tests import hop_outgoing_cases as HC
from tests import hop_outgoing_numpy as HO

pytestmark = pytest.mark.gpu
N_TRAJ, MASS, LEFT, RIGHT, SEED, N_BINS = HC.N_TRAJ, HC.MASS, HC.LEFT, HC.RIGHT, HC.SEED, HC.N_BINS
BAD_ARG = 1
TWO32 = 4294967296
WIDE = (-1000.0, 2000.0 / 63.0, 64)  # a momentum grid nothing is outside of
_states = {}


@pytest.fixture
def model_of(gpu):
    ids = []

    def make(c):
        if not c["tabulated"]:
            return c["model"]
        t = HC.tabulated(c["model"], c["N"])
        ids.append(gpu.pes_define(c["N"], t.x_first, t.dx, t.V, t.dV))
        return ids[-1]

    yield make
    for model in ids:
        gpu.pes_undefine(model)


def state_of(gpu, name, kind, model):
    """the device's own ensemble of the case and kind, on the host; made once"""
    if (name, kind) not in _states:
        c = HC.case_of(name)
        N, (_, window, gamma) = c["N"], HC.KINDS[kind]
        if kind in ("fssh", "ehrenfest"):
            start = gpu.hop_sample(N, model, N_TRAJ, SEED, *HC.packet(c["p0"]), c["surface0"])
        else:
            start = gpu.hop_sample_sqc(N, model, N_TRAJ, SEED, *HC.packet(c["p0"]), c["surface0"], window, gamma)
        if kind == "fssh":
            end = gpu.hop_evolve(N, model, start, SEED, MASS, c["dt"], 0, c["steps"], LEFT, RIGHT)
        elif kind == "ehrenfest":
            end = gpu.hop_evolve_mf(N, model, start, MASS, c["dt"], c["steps"], LEFT, RIGHT)
        else:
            end = gpu.hop_evolve_sqc(N, model, start, MASS, c["dt"], c["steps"], LEFT, RIGHT, gamma)
        _states[(name, kind)] = tuple(np.array(a) for a in end)
    return _states[(name, kind)]


def device_call(gpu, kind, N, model, state, grid, axis, acc=None):
    form, window, gamma = HC.KINDS[kind]
    if form == "surface":
        return gpu.hop_outgoing(N, model, state, MASS, grid, axis, acc=acc)
    if form == "amplitude":
        return gpu.hop_outgoing_mf(N, model, state, MASS, grid, axis, acc=acc)
    return gpu.hop_outgoing_sqc(N, model, state, MASS, grid, axis, window, gamma, acc=acc)


def restated(kind, c, state, grid, axis, **kw):
    form, window, gamma = HC.KINDS[kind]
    return HO.outgoing(form, c["potential"], state, MASS, grid, axis, window, gamma, **kw)


def to_device(gpu, arrays):
    import torch

    where = torch.device("cuda", gpu.device)
    out = tuple(torch.from_numpy(np.array(a)).to(where) for a in arrays)
    torch.cuda.synchronize(where)
    return out


def planes_of(acc, N):
    return acc[:-4].reshape(2, N, -1)


def grids_of(kind, c, state):
    form, window, gamma = HC.KINDS[kind]
    return {"momentum": HC.momentum_grid(c["p0"]), "energy": HC.energy_grid(form, c["potential"], state, window, gamma)}


def the_case_tests_something(acc, N, state):
    assert (planes_of(acc, N).sum(axis=2) > 0).sum() >= 2 and acc[-2] == (state[4] == 0).sum() >= 1 and acc[-4] > 0


def assert_equal_but_aside(got, kind, c, state, grid, axis, aside):
    """every word EQUAL; with trajectories set aside (at most two): the rest equal, and what they added sits in their side's planes within one
    bin of where the restatement puts them (any level: a window edge decides the level), or in a tally"""
    want = restated(kind, c, state, grid, axis)
    if not aside.any():
        assert np.array_equal(got, want)
        return
    N, parts = c["N"], {}
    rest = restated(kind, c, state, grid, axis, skip=aside, parts=parts)
    extra = got - rest
    allowed = np.zeros((2, N, grid[2]), dtype=bool)
    for i in np.nonzero(aside)[0]:
        j = int(parts["j"][i])
        allowed[int(parts["side"][i]), :, max(j - 1, 0):j + 2] = True
    assert (extra >= 0).all() and not planes_of(extra, N)[~allowed].any()
    assert planes_of(extra, N).sum() == TWO32 * extra[-4] and extra[-4] + extra[-3] + extra[-1] == aside.sum() and extra[-2] == 0


# ---- 1, 2, 4. the surface and the window form: every word -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(HC.CASES))
@pytest.mark.parametrize("kind", ["fssh", "square", "triangle"])
def test_every_word_against_the_restatement(gpu, model_of, name, kind):
    c = HC.case_of(name)
    N, model = c["N"], model_of(c)
    form, window, gamma = HC.KINDS[kind]
    state = state_of(gpu, name, kind, model)
    for axis, grid in grids_of(kind, c, state).items():
        aside, m = HC.set_aside(form, c["potential"], state, grid, axis, window, gamma)
        assert aside.sum() <= HC.MOST_ASIDE
        assert axis == "energy" or form == "window" or not aside.any()  # 1: surface form, momentum axis: nothing is set aside
        got = device_call(gpu, kind, N, model, state, grid, axis)
        assert got.dtype == np.int64 and got.shape == (HO.words(N, N_BINS),)
        the_case_tests_something(got, N, state)
        print(f"hop outgoing {name} {kind} {axis}: tallies {list(got[-4:])}, set aside {int(aside.sum())}, least edge distance {m['edge'].min():.3g} step, "
              f"least window distance {m['window'].min():.3g}")
        assert_equal_but_aside(got, kind, c, state, grid, axis, aside)
        assert got[-1] == 0 or form == "window"


# ---- 3. the amplitude form ----------------------------------------------------------------------------------------------------------------------------
def assert_amplitude_words(label, got, potential, N, state, grid, axis):
    """the acc of an amplitude-form call against the restatement on `state` (host arrays): `running` and `unassigned` equal and `binned +
    outside` equal always (a trajectory set aside can only move between those two, at the outer edge of the grid), all four equal where none
    is set aside; every word within the sum over the restatement's trajectories of that word of 2^32 (64 D_w + 1e-13) + 1, D_w the float64
    against long double difference of that trajectory's weight of that level; a trajectory set aside may have its whole weight in either
    neighbouring bin"""
    n_bins = grid[2]
    aside, m = HC.set_aside("amplitude", potential, state, grid, axis)
    assert aside.sum() <= HC.MOST_ASIDE and (axis == "energy" or not aside.any())
    parts = {}
    want = HO.outgoing("amplitude", potential, state, MASS, grid, axis, parts=parts)
    assert np.array_equal(got[-2:], want[-2:]) and got[-4] + got[-3] == want[-4] + want[-3]
    if not aside.any():
        assert np.array_equal(got[-4:], want[-4:])
    bound = np.zeros((2, N, n_bins))
    for i in np.nonzero(parts["finished"] & (parts["j"] >= 0))[0]:
        side, j = int(parts["side"][i]), int(parts["j"][i])
        term = TWO32 * (64.0 * m["D_w"][i] + 1e-13) + 1.0
        bound[side, :, j] += term
        if aside[i]:
            bound[side, :, max(j - 1, 0):j + 2] += (TWO32 * parts["w"][i] + term)[:, None]
    off = np.abs(planes_of(got, N) - planes_of(want, N))
    print(f"{label}: tallies {[int(v) for v in got[-4:]]}, set aside {int(aside.sum())}, the largest difference of a word is {int(off.max())} unit(s) of 2^-32 "
          f"where the bound allows {bound[off == off.max()].min():.3g}, the least slack of a word is {(bound - off).min():.3g}, D_w <= {m['D_w'].max():.3g}")
    assert (off <= bound).all()


@pytest.mark.parametrize("name", list(HC.CASES))
def test_the_amplitude_form_against_the_restatement(gpu, model_of, name):
    c = HC.case_of(name)
    N, model = c["N"], model_of(c)
    state = state_of(gpu, name, "ehrenfest", model)
    for axis, grid in grids_of("ehrenfest", c, state).items():
        got = device_call(gpu, "ehrenfest", N, model, state, grid, axis)
        the_case_tests_something(got, N, state)
        assert_amplitude_words(f"hop outgoing_mf {name} {axis}", got, c["potential"], N, state, grid, axis)


# ---- 5. crowding and tails ----------------------------------------------------------------------------------------------------------------------------
def crowd(n, running):
    """n trajectories at one point of phase space on surface 1, all gone to the right but the first `running`"""
    b = np.zeros((n, 2), dtype=np.complex128)
    b[:, 0] = 1.0
    status = np.full(n, 2, dtype=np.int32)
    status[:running] = 0
    return np.full(n, 7.0), np.full(n, 11.0), b, np.ones(n, dtype=np.int32), status


@pytest.mark.parametrize("running", [0, 2049])
def test_every_add_to_one_word(gpu, running):
    n = 4099
    state = crowd(n, running)
    energy = float(HO.classify("surface", HN.builtin(HN.DAC, 2), state, MASS)["energy"][-1])
    for axis, grid, j in (("momentum", HC.momentum_grid(10.0), int(np.floor((11.0 + 20.0) / (40.0 / 63.0) + 0.5))), ("energy", (energy - 1.0, 0.25, N_BINS), 4)):
        got = gpu.hop_outgoing(2, HN.DAC, state, MASS, grid, axis)
        want = np.zeros(HO.words(2, N_BINS), dtype=np.int64)
        want[(1 * 2 + 1) * N_BINS + j] = (n - running) * TWO32
        want[-4], want[-2] = n - running, running
        assert np.array_equal(got, want), (axis, got[-4:], np.nonzero(got)[0])


# ---- 6. bits ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, kind", [("tsac", "fssh"), ("tsac", "ehrenfest"), ("tsac", "square"), ("dac10", "triangle"), ("table2", "fssh")])
def test_bits(gpu, model_of, name, kind):
    c = HC.case_of(name)
    N, model = c["N"], model_of(c)
    form = HC.KINDS[kind][0]
    state = state_of(gpu, name, kind, model)
    finished = int(((state[4] == 1) | (state[4] == 2)).sum())
    for axis, grid in grids_of(kind, c, state).items():
        whole = device_call(gpu, kind, N, model, state, grid, axis)
        assert np.array_equal(device_call(gpu, kind, N, model, state, grid, axis), whole)                      # a repeat
        on_device = to_device(gpu, state)                                                                    # device pointers
        acc = device_call(gpu, kind, N, model, on_device, grid, axis)
        gpu.synchronize()
        assert acc.is_cuda and np.array_equal(acc.cpu().numpy(), whole)
        part = device_call(gpu, kind, N, model, tuple(a[:150] for a in state), grid, axis)                   # two slices, the second accumulated
        assert not np.array_equal(part, whole)
        assert np.array_equal(device_call(gpu, kind, N, model, tuple(a[150:] for a in state), grid, axis, acc=part), whole)
        part_d = device_call(gpu, kind, N, model, tuple(a[:150].contiguous() for a in on_device), grid, axis)
        both_d = device_call(gpu, kind, N, model, tuple(a[150:].contiguous() for a in on_device), grid, axis, acc=part_d)
        gpu.synchronize()
        assert both_d is part_d and np.array_equal(both_d.cpu().numpy(), whole)
        one = device_call(gpu, kind, N, model, state, (grid[0] + 31.5 * grid[1], 64.0 * grid[1], 1), axis)    # n_bins = 1: one word per plane
        assert one.shape == (2 * N + 4,) and np.array_equal(one[-4:], whole[-4:]) and np.array_equal(one[:-4], planes_of(whole, N).sum(axis=2).reshape(-1))
        nothing = device_call(gpu, kind, N, model, state, (grid[0] - 1e6 * grid[1], grid[1], N_BINS), axis)   # a grid that covers nothing
        assert not nothing[:-4].any() and nothing[-4] == 0 and nothing[-3] == finished - whole[-1] and np.array_equal(nothing[-2:], whole[-2:])
    # a NaN p is outside; a status of 7 and (where it is read) a surface of -1 are skipped
    grid = HC.momentum_grid(c["p0"])
    whole = device_call(gpu, kind, N, model, state, grid, "momentum")
    assigned = np.nonzero(HO.classify(form, c["potential"], state, MASS, *HC.KINDS[kind][1:])["level"] >= 0)[0] if form != "amplitude" else np.nonzero(state[4] > 0)[0]
    odd = tuple(np.array(a) for a in state)
    odd[1][assigned[0]] = np.nan
    got = device_call(gpu, kind, N, model, odd, grid, "momentum")
    assert got[-3] == whole[-3] + 1 and got[-4] == whole[-4] - 1 and (form == "amplitude" or np.array_equal(got, restated(kind, c, odd, grid, "momentum")))
    odd[4][assigned[1]] = 7
    odd[3][assigned[2]] = -1
    got = device_call(gpu, kind, N, model, odd, grid, "momentum")
    assert got[-4] == whole[-4] - (3 if form == "surface" else 2) and got[-3] == whole[-3] + 1 and np.array_equal(got[-2:], whole[-2:])
    if form != "amplitude":
        assert np.array_equal(got, restated(kind, c, odd, grid, "momentum"))


# ---- 7. against the device's own sums -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(HC.CASES))
def test_the_planes_add_up_to_the_counts_of_the_device_sums(gpu, model_of, name):
    c = HC.case_of(name)
    N, model = c["N"], model_of(c)
    state = state_of(gpu, name, "fssh", model)
    got = gpu.hop_outgoing(N, model, state, MASS, WIDE, "momentum")
    counts = np.rint(gpu.hop_observe(N, model, state, MASS)[:3 * N]).astype(np.int64).reshape(3, N)
    assert got[-3] == 0 and np.array_equal(planes_of(got, N).sum(axis=2), TWO32 * counts[1:]) and got[-2] == counts[0].sum()
    for kind in ("square", "triangle"):
        _, window, gamma = HC.KINDS[kind]
        state = state_of(gpu, name, kind, model)
        got = gpu.hop_outgoing_sqc(N, model, state, MASS, WIDE, "momentum", window, gamma)
        sums = np.rint(gpu.hop_observe_sqc(N, model, state, MASS, window, gamma)).astype(np.int64)
        assert got[-3] == 0 and np.array_equal(planes_of(got, N).sum(axis=2), TWO32 * sums[N:3 * N].reshape(2, N))
        assert got[-2] == sums[3 * N] and got[-1] == sums[3 * N + 4] + sums[3 * N + 5]
    state = state_of(gpu, name, "ehrenfest", model)
    got = gpu.hop_outgoing_mf(N, model, state, MASS, WIDE, "momentum")
    sums = gpu.hop_observe_mf(N, model, state, MASS)
    # a weight is rounded to half a unit, and the float sums of the observe call to 1e-12 a term
    assert (np.abs(planes_of(got, N).sum(axis=2) - TWO32 * sums[N:3 * N].reshape(2, N)) <= sums[3 * N + 1:3 * N + 3, None] * (0.5 + TWO32 * 1e-12)).all()
    assert list(got[-4:]) == [sums[3 * N + 1] + sums[3 * N + 2], 0, sums[3 * N], 0]


# ---- 8. GPLE_ERR_BAD_ARG --------------------------------------------------------------------------------------------------------------------------------
def test_a_refused_call_writes_nothing(gpu):
    state = state_of(gpu, "dac10", "fssh", HN.DAC)
    x, p, b, surface, status = (a.copy() for a in state)
    dp_, ip, llp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_longlong)
    arrays = dict(x=x.ctypes.data_as(dp_), p=p.ctypes.data_as(dp_), b=b.ctypes.data_as(dp_), surface=surface.ctypes.data_as(ip), status=status.ctypes.data_as(ip))
    pattern = np.arange(HO.words(2, N_BINS), dtype=np.int64) * 7 - 1000
    acc = pattern.copy()
    nan, inf = float("nan"), float("inf")
    lib, ctx = gpu.lib, gpu.ctx

    def call(entry, **kw):
        a = dict(num_pes=2, model=1, n=N_TRAJ, mass=MASS, window=1, gamma=1.0 / 3.0, axis=0, first=-20.0, step=40.0 / 63.0, n_bins=N_BINS, flags=0,
                 acc=acc.ctypes.data_as(llp), **arrays)
        a.update(kw)
        head = (ctx, a["num_pes"], a["model"], a["n"], a["mass"])
        rest = (a["axis"], a["first"], a["step"], a["n_bins"], a["flags"], a["x"], a["p"], a["b"])
        if entry == "surface":
            return lib.gple_hop_outgoing(*head, *rest, a["surface"], a["status"], a["acc"])
        if entry == "amplitude":
            return lib.gple_hop_outgoing_mf(*head, *rest, a["status"], a["acc"])
        return lib.gple_hop_outgoing_sqc(*head, a["window"], a["gamma"], *rest, a["status"], a["acc"])

    shared = [dict(num_pes=1), dict(num_pes=4), dict(model=-1), dict(model=7), dict(model=_capi.PES_USER + 15), dict(n=0), dict(n=(1 << 31) + 1), dict(n=1 << 32),
              dict(mass=0.0), dict(mass=-1.0), dict(mass=nan), dict(mass=inf), dict(axis=-1), dict(axis=2), dict(n_bins=0), dict(n_bins=(1 << 28) // 6 + 1),
              dict(n_bins=1 << 62), dict(step=0.0), dict(step=-1.0), dict(step=nan), dict(step=inf), dict(first=nan), dict(first=-inf), dict(acc=None),
              dict(x=None), dict(p=None), dict(b=None), dict(status=None)]
    for kw in shared + [dict(surface=None)]:
        assert call("surface", **kw) == BAD_ARG, kw
    for kw in shared:
        assert call("amplitude", **kw) == BAD_ARG, kw
    for kw in shared + [dict(window=2), dict(window=-1), dict(gamma=nan), dict(gamma=-0.1), dict(window=0, gamma=0.5), dict(window=0, gamma=0.0),
                        dict(flags=_capi.HOP_REVERSE)]:
        assert call("window", **kw) == BAD_ARG, kw
    assert np.array_equal(acc, pattern)  # a refused call writes nothing
    want = {form: HO.outgoing(form, HN.builtin(HN.DAC, 2), state, MASS, HC.momentum_grid(10.0), 0, 1, 1.0 / 3.0) for form in HO.FORMS}
    for entry in ("surface", "window"):  # and the same arguments are taken: without the flag acc is cleared first, with it the call adds
        assert call(entry) == 0 and np.array_equal(acc, want[entry])
        assert call(entry, flags=_capi.HOP_ACCUMULATE) == 0 and np.array_equal(acc, 2 * want[entry])
    assert call("amplitude") == 0 and np.array_equal(acc[-4:], want["amplitude"][-4:])


# ---- the timer ------------------------------------------------------------------------------------------------------------------------------------------
def test_the_timer_counts_the_calls_of_all_three(gpu):
    state = state_of(gpu, "dac10", "fssh", HN.DAC)
    grid = HC.momentum_grid(10.0)
    gpu.enable_timing(True)
    try:
        before = gpu.timing(_capi.TIMER_HOP_OUTGOING)[2], gpu.timing(_capi.TIMER_HOP_BIN)[2]
        gpu.hop_outgoing(2, HN.DAC, state, MASS, grid)
        gpu.hop_outgoing_mf(2, HN.DAC, state, MASS, grid, "energy")
        gpu.hop_outgoing_sqc(2, HN.DAC, state, MASS, grid)
        last, _, count = gpu.timing(_capi.TIMER_HOP_OUTGOING)
        assert count == before[0] + 3 and last > 0.0 and gpu.timing(_capi.TIMER_HOP_BIN)[2] == before[1]
    finally:
        gpu.enable_timing(False)


# ---- 9. the driver --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["fssh", "mash", "ehrenfest"])
def test_the_driver_against_the_stand_in(gpu, tmp_path, method):
    """t = 0, 430, 860: the centre of the packet is at the right bound"""
    kw = dict(model=hopping.DAC, num_pes=2, ln_energy=-2.0, n_traj=512, seed=SEED, dt=4.0, x0=HC.X0, xmin=LEFT, xmax=RIGHT, output_time=430.0, max_outputs=3,
              method=method, outgoing={"momentum": 64, "energy": 32})
    res = hopping.run(gpu, out_dir=str(tmp_path / "device"), **kw)
    ref = hopping.run(HO.APIS[method](), out_dir=str(tmp_path / "numpy"), **kw)
    assert res["state"][0].is_cuda and list(res["outgoing"]) == list(ref["outgoing"]) == ["momentum", "energy"]
    for axis, name in (("momentum", "outgoing_p.txt"), ("energy", "outgoing_e.txt")):
        got, want = res["outgoing"][axis], ref["outgoing"][axis]
        assert got["acc"].is_cuda and np.allclose(got["grid"], want["grid"], rtol=1e-13, atol=0) and got["grid"][2] == want["grid"][2]
        acc = got["acc"].cpu().numpy()
        assert acc[-4] > 50 and acc[-2] > 50 and acc[-3] == 0
        if method == "ehrenfest":
            # item 3's bound, word by word, on the stand-in's final state and grid
            assert_amplitude_words(f"hop outgoing_mf driver {axis}", acc, HN.builtin(HN.DAC, 2), 2, ref["state"], want["grid"], axis)
            assert np.array_equal(HO.outgoing("amplitude", HN.builtin(HN.DAC, 2), ref["state"], MASS, want["grid"], axis), want["acc"])
        else:
            assert np.array_equal(acc, want["acc"]) and got["tallies"] == want["tallies"]
            assert np.allclose(got["density"], want["density"], rtol=1e-13, atol=0)  # the default grids come from the adiabatic energies of either side
            assert (tmp_path / "device" / name).read_text() == (tmp_path / "numpy" / name).read_text()
        assert got["density"].shape == (2, 2, got["grid"][2]) and (tmp_path / "device" / name).exists()
