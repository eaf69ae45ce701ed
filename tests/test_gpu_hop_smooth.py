"""GPU: the smoothed phase-space density of an ensemble (gple_hop_smooth / gple_hop_smooth_mf, csrc/gple_hop.hip; DESIGN.md §17 "The ensemble in
phase space, smoothed") against the long double restatement tests/hop_smooth_numpy.py.  Every test fails without the feature.

Every state is the DEVICE's own ensemble (tests/hop_smooth_cases.py), copied to the host: the same arrays go to the call and to the
restatement.  |device - long double| <= B for every entry of every plane, B the bound of the restatement's text, and the tallies are EQUAL.  No
entry and no trajectory is set aside: the kernel takes no discrete decision but the selection, which is exact.  The precondition that no sign
convention of an eigenvector can flip between the two is asserted.

Worst error over bound measured on the MI355X (pytest -s prints them): 0.499 over the evolved ensembles (the table of DAC, running trajectories
only; the float64 restatement on the host reaches the same 0.499 there: it is the rounding of the weights, not of the contraction), 0.06 over the
chunk edges."""
import ctypes as C

import numpy as np
import pytest

from gaussian_process_liouville_equation_amd import _capi, hopping, reconstruct
from tests import hop_numpy as HN
from tests import hop_outgoing_cases as HOC
from tests import hop_smooth_cases as SC
from tests import hop_smooth_numpy as HS

pytestmark = pytest.mark.gpu
BAD_ARG = 1
_states = {}


@pytest.fixture
def model_of(gpu):
    ids = []

    def make(c):
        if not c["tabulated"]:
            return c["model"]
        t = HOC.tabulated(c["model"], c["N"])
        ids.append(gpu.pes_define(c["N"], t.x_first, t.dx, t.V, t.dV))
        return ids[-1]

    yield make
    for model in ids:
        gpu.pes_undefine(model)


def state_of(gpu, name, model):
    """the device's own ensemble of the case, on the host; made once"""
    if name not in _states:
        case, kind = SC.ENSEMBLES[name]
        c = HOC.case_of(case)
        start = gpu.hop_sample(c["N"], model, HOC.N_TRAJ, HOC.SEED, *HOC.packet(c["p0"]), c["surface0"])
        if kind == "ehrenfest":
            _states[name] = gpu.hop_evolve_mf(c["N"], model, start, HOC.MASS, c["dt"], c["steps"], HOC.LEFT, HOC.RIGHT)
        else:
            _states[name] = gpu.hop_evolve(c["N"], model, start, HOC.SEED, HOC.MASS, c["dt"], 0, c["steps"], HOC.LEFT, HOC.RIGHT)
    return _states[name]


def to_device(gpu, arrays):
    import torch

    where = torch.device("cuda", gpu.device)
    out = tuple(torch.from_numpy(np.array(a)).to(where) for a in arrays)
    torch.cuda.synchronize(where)
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.float64).view(np.uint64)


def call(gpu, mean_field):
    return gpu.hop_smooth_mf if mean_field else gpu.hop_smooth


# ---- 1. every entry of every plane against long double ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mean_field,bin_all", SC.FORMS)
@pytest.mark.parametrize("name", list(SC.ENSEMBLES))
def test_against_long_double(gpu, model_of, name, mean_field, bin_all):
    c = HOC.case_of(SC.ENSEMBLES[name][0])
    N, model = c["N"], model_of(c)
    state = state_of(gpu, name, model)
    assert all((state[4] == s).any() for s in (0, 1, 2)), "the case has lost a status"
    assert SC.signs_are_safe(c["potential"], state, mean_field, bin_all)
    worst = 0.0
    for label, grid, h in SC.configurations(state):
        rho, tallies = call(gpu, mean_field)(N, model, state, grid, h, SC.N_TRAJ, bin_all=bin_all)
        assert rho.shape == (N, N, grid[2], grid[5]) and tallies[0] == (SC.N_TRAJ if bin_all else (state[4] == 0).sum()) and tallies[1] == 0
        worst = max(worst, SC.check(rho, tallies, ("device", name, label, mean_field, bin_all), c["potential"], state, grid, h, SC.N_TRAJ, mean_field, bin_all))
        for a in range(N):
            assert not bits(rho[a, a].imag).any()  # +0 exactly
            for b in range(a + 1, N):
                assert np.array_equal(rho[b, a], np.conj(rho[a, b]))  # -0 only where s times a tiny negated sum underflows
    print(f"hop smooth {name} mean_field={mean_field} bin_all={bin_all}: the worst error over bound is {worst:.3f}")
    assert worst > 0.0


# ---- 2. the edges of the trajectory chunks ----------------------------------------------------------------------------------------------------
def split_of(gpu, N, n, n_x, n_p):
    chunk, n_chunks = C.c_size_t(0), C.c_size_t(0)
    fn = gpu.lib.gple_debug_hop_smooth_split
    fn.argtypes, fn.restype = [C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)], C.c_int
    assert fn(N, n, n_x, n_p, C.byref(chunk), C.byref(n_chunks)) == 0
    return chunk.value, n_chunks.value


@pytest.mark.parametrize("case", ["dac10", "tsac"])
def test_chunk_edges(gpu, case):
    """n = CH - 1, CH, CH + 1, 2 CH + 3 and one more n that is no multiple of 4, CH the trajectories of a chunk as the library's rule gives them
    on 17 x 19: sampled x and p with synthetic statuses, surfaces and unit amplitudes (a fresh sample sits on one adiabatic state, where every
    coherence is rounding noise)"""
    c = HOC.case_of(case)
    N, model = c["N"], c["model"]
    CH, _ = split_of(gpu, N, 1, 17, 19)
    assert 16 <= CH <= 4096 and CH % 16 == 0
    rng = np.random.default_rng(12)
    worst, seen = 0.0, set()
    for n in (CH - 1, CH, CH + 1, 2 * CH + 3, CH + 45):
        chunk, n_chunks = split_of(gpu, N, n, 17, 19)
        assert chunk == CH and n_chunks == -(-n // CH)
        seen.add(n_chunks)
        x, p, _, _, _ = gpu.hop_sample(N, model, n, HOC.SEED, *HOC.packet(c["p0"]), c["surface0"])
        b = rng.normal(size=(n, N)) + 1j * rng.normal(size=(n, N))
        b /= np.linalg.norm(b, axis=1)[:, None]
        state = (x, p, b, rng.integers(0, N, n).astype(np.int32), rng.integers(0, 3, n).astype(np.int32))
        grid = SC.grid_over(state, 17, 19)
        h = (1.5 * grid[1], 1.5 * grid[4])
        for mean_field, bin_all in SC.FORMS:
            assert SC.signs_are_safe(c["potential"], state, mean_field, bin_all)
            rho, tallies = call(gpu, mean_field)(N, model, state, grid, h, n, bin_all=bin_all)
            worst = max(worst, SC.check(rho, tallies, ("edges", case, n, mean_field, bin_all), c["potential"], state, grid, h, n, mean_field, bin_all))
    assert (CH + 45) % 4 and seen == {1, 2, 3}
    print(f"hop smooth chunk edges {case}: CH = {CH}, the worst error over bound is {worst:.3f}")


# ---- 3. bits and edges ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dac10-fssh", "tsac", "table2"])
def test_bits(gpu, model_of, name):
    c = HOC.case_of(SC.ENSEMBLES[name][0])
    N, model = c["N"], model_of(c)
    state = state_of(gpu, name, model)
    on_device = to_device(gpu, state)
    for shape in ((24, 40), (65, 17)):
        grid = SC.grid_over(state, *shape)
        h = (1.5 * grid[1], 1.5 * grid[4])
        for mean_field in (False, True):
            whole, tallies = call(gpu, mean_field)(N, model, state, grid, h, SC.N_TRAJ, bin_all=True)
            again, tallies2 = call(gpu, mean_field)(N, model, state, grid, h, SC.N_TRAJ, bin_all=True)                  # a repeat
            assert np.array_equal(bits(again), bits(whole)) and tallies2 == tallies == (SC.N_TRAJ, 0)
            rho, tallies3 = call(gpu, mean_field)(N, model, on_device, grid, h, SC.N_TRAJ, bin_all=True)                 # device pointers
            gpu.synchronize()
            assert rho.is_cuda and tallies3 == tallies and np.array_equal(bits(rho.cpu().numpy()), bits(whole))
            if mean_field:                                                                                               # the surface is not read
                odd = (state[0], state[1], state[2], np.full(SC.N_TRAJ, 7, dtype=np.int32), state[4])
                assert np.array_equal(bits(gpu.hop_smooth_mf(N, model, odd, grid, h, SC.N_TRAJ, bin_all=True)[0]), bits(whole))


def test_nobody_selected_and_a_nan(gpu):
    c = HOC.case_of("dac10")
    state = state_of(gpu, "dac10-fssh", c["model"])
    grid = SC.grid_over(state, 24, 40)
    h = (1.5 * grid[1], 1.5 * grid[4])
    nobody = (state[0], state[1], state[2], state[3], np.full(SC.N_TRAJ, 7, dtype=np.int32))
    for mean_field in (False, True):
        rho, tallies = call(gpu, mean_field)(2, c["model"], nobody, grid, h, SC.N_TRAJ, bin_all=True)
        assert tallies == (0, 0) and not bits(rho).any()  # all +0
    x, p = state[0].copy(), state[1].copy()
    running = np.flatnonzero(state[4] == 0)
    p[running[0]], x[running[1]], p[running[2]] = np.nan, np.inf, -np.inf
    holed = (x, p, state[2], state[3], state[4])
    for mean_field, bin_all in SC.FORMS:
        rho, tallies = call(gpu, mean_field)(2, c["model"], holed, grid, h, SC.N_TRAJ, bin_all=bin_all)
        assert tallies == ((SC.N_TRAJ if bin_all else len(running)) - 3, 3)
        SC.check(rho, tallies, ("holed", mean_field, bin_all), c["potential"], holed, grid, h, SC.N_TRAJ, mean_field, bin_all)
        keep = np.ones(SC.N_TRAJ, dtype=bool)
        keep[running[:3]] = False
        without, _ = call(gpu, mean_field)(2, c["model"], tuple(np.ascontiguousarray(a[keep]) for a in state), grid, h, SC.N_TRAJ, bin_all=bin_all)
        assert np.abs(rho - without).max() <= 1e-12 * np.abs(without).max()  # the three contribute nothing


# ---- 4. GPLE_ERR_BAD_ARG ----------------------------------------------------------------------------------------------------------------------
def test_bad_arguments(gpu):
    import gaussian_process_liouville_equation_amd as pkg

    state = state_of(gpu, "dac10-fssh", HN.DAC)
    x, p, b, surface, status = (a.copy() for a in state)
    dp_, ip, llp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_longlong)
    arrays = dict(x=x.ctypes.data_as(dp_), p=p.ctypes.data_as(dp_), b=b.ctypes.data_as(dp_), surface=surface.ctypes.data_as(ip), status=status.ctypes.data_as(ip))
    rho = np.full(2 * 4 * 16 * 9, -7.0)
    tally = np.full(2, -7, dtype=np.int64)
    nan, inf = float("nan"), float("inf")
    lib, ctx = gpu.lib, gpu.ctx

    def smooth(mean_field, **kw):
        a = dict(num_pes=2, model=1, n=SC.N_TRAJ, x_first=-6.0, dx=0.8, n_x=16, p_first=0.0, dp=3.75, n_p=9, h_x=1.0, h_p=4.0, n_norm=SC.N_TRAJ, flags=0,
                 rho=rho.ctypes.data_as(dp_), tally=tally.ctypes.data_as(llp), **arrays)
        a.update(kw)
        head = (ctx, a["num_pes"], a["model"], a["n"], a["x_first"], a["dx"], a["n_x"], a["p_first"], a["dp"], a["n_p"], a["h_x"], a["h_p"], a["n_norm"], a["flags"],
                a["x"], a["p"], a["b"])
        if mean_field:
            return lib.gple_hop_smooth_mf(*head, a["status"], a["rho"], a["tally"])
        return lib.gple_hop_smooth(*head, a["surface"], a["status"], a["rho"], a["tally"])

    table = HOC.tabulated(HN.DAC, 2)
    mine = gpu.pes_define(2, table.x_first, table.dx, table.V, table.dV)
    other = pkg.open_api(0)
    try:
        theirs = other.pes_define(2, table.x_first, table.dx, table.V, table.dV)
        theirs = other.pes_define(2, table.x_first, table.dx, table.V, table.dV)  # a second slot, free on the session's context
        assert theirs != mine
        bad = [dict(num_pes=1), dict(num_pes=4), dict(model=-1), dict(model=3), dict(model=7), dict(model=_capi.PES_USER + 15), dict(model=theirs),
               dict(model=mine, num_pes=3), dict(n=0), dict(n=(1 << 31) + 1), dict(n=1 << 32), dict(x_first=nan), dict(x_first=inf), dict(p_first=nan),
               dict(p_first=-inf), dict(n_x=0), dict(n_p=0), dict(n_x=(1 << 28) + 1, n_p=1), dict(n_x=1 << 15, n_p=(1 << 13) + 1), dict(n_x=1 << 62, n_p=4),
               dict(dx=0.0), dict(dx=-1.0), dict(dx=nan), dict(dx=inf), dict(dp=0.0), dict(dp=-1.0), dict(dp=nan), dict(dp=inf), dict(n_norm=0),
               dict(h_x=0.0), dict(h_x=-1.0), dict(h_x=nan), dict(h_x=inf), dict(h_p=0.0), dict(h_p=-2.0), dict(h_p=nan), dict(h_p=inf),
               dict(h_x=1e-200, h_p=1e-200), dict(h_x=1e200, h_p=1e200),                                     # s is infinite, s is 0
               dict(flags=_capi.HOP_ACCUMULATE), dict(flags=0x2000), dict(flags=_capi.HOP_BIN_ALL | 0x2000), dict(rho=None)]
        for mean_field in (False, True):
            for kw in bad + [{k: None} for k in arrays if not (mean_field and k == "surface")]:
                assert smooth(mean_field, **kw) == BAD_ARG, (mean_field, kw)
        assert (rho == -7.0).all() and (tally == -7).all()  # a refused call writes nothing
        for mean_field in (False, True):
            tally[:] = -7
            assert smooth(mean_field, model=mine, tally=None) == 0 and np.isfinite(rho).all() and (tally == -7).all()  # tally is nullable
            assert smooth(mean_field, flags=_capi.HOP_BIN_ALL) == 0 and list(tally) == [SC.N_TRAJ, 0]
    finally:
        other.close()
        gpu.pes_undefine(mine)


# ---- 5. the timer -------------------------------------------------------------------------------------------------------------------------------
def test_the_timer_counts_the_calls(gpu):
    state = state_of(gpu, "dac10-fssh", HN.DAC)
    grid = SC.grid_over(state, 24, 40)
    gpu.enable_timing(True)
    try:
        before = gpu.timing(_capi.TIMER_HOP_SMOOTH)[2], gpu.timing(_capi.TIMER_HOP_BIN)[2]
        gpu.hop_smooth(2, HN.DAC, state, grid, (grid[1], grid[4]), SC.N_TRAJ)
        gpu.hop_smooth_mf(2, HN.DAC, state, grid, (grid[1], grid[4]), SC.N_TRAJ)
        last, _, count = gpu.timing(_capi.TIMER_HOP_SMOOTH)
        assert count == before[0] + 2 and last > 0.0 and gpu.timing(_capi.TIMER_HOP_BIN)[2] == before[1]
    finally:
        gpu.enable_timing(False)


# ---- 6. the driver ------------------------------------------------------------------------------------------------------------------------------
def test_driver_against_the_stand_in(gpu, tmp_path):
    kw = dict(n_traj=512, ln_energy=-2.0, phase_grid=(24, 40), phase_smooth="scott", max_outputs=4)
    res = hopping.run(gpu, out_dir=str(tmp_path / "device"), **kw)
    api = HS.NumpyHopSmoothApi()
    ref = hopping.run(api, out_dir=str(tmp_path / "numpy"), **kw)
    assert len(res["records"]) == len(ref["records"]) == 4 and res["state"][0].is_cuda and res["phase_smooth"] == ref["phase_smooth"]
    for name in ("x.txt", "p.txt", "t.txt"):
        assert (tmp_path / "device" / name).read_text() == (tmp_path / "numpy" / name).read_text()
    s, h = ref["setup"], ref["phase_smooth"]
    grid = hopping.phase_grid_of(api, 2, hopping.DAC, s, (24, 40))
    pot = HN.builtin(HN.DAC, 2)
    blocks = [list(reconstruct.phase_blocks(str(tmp_path / d / "phase.txt"), 2, 24, 40)) for d in ("device", "numpy")]
    assert len(blocks[0]) == len(blocks[1]) == 4
    state = HN.sample(pot, 2, 512, 0, s["x0"], s["p0"], s["sigma_x"], s["sigma_p"], 0)  # the stand-in's states again, for B
    for k, (a, b, got, want) in enumerate(zip(res["records"], ref["records"], *blocks)):
        assert a["t"] == b["t"] and (a["binned"], a["outside"]) == (b["binned"], b["outside"]) and np.array_equal(a["binned_counts"], b["binned_counts"])
        assert (a["smoothed"], a["nonfinite"]) == (b["smoothed"], b["nonfinite"]) == (int(a["counts"][hopping.RUNNING].sum()), 0) and a["smoothed"] > 0
        assert np.array_equal(a["counts"], b["counts"])
        got, want = (reconstruct._parse_host(block)[0].view(np.complex128).reshape(2, 2, 24, 40) for block in (got, want))
        _, _, B = HS.smooth(pot, state, grid, h, 512, dtype=np.longdouble, with_bound=True)
        # "%g" on either side: 5e-6 of the value each; B for the device against long double and once more for the stand-in against it
        tol = 1.1e-5 * np.abs(want.view(np.float64).reshape(2, 2, 24, 40, 2)) + 2.0 * B.astype(np.float64)
        assert (np.abs(got.view(np.float64) - want.view(np.float64)).reshape(2, 2, 24, 40, 2) <= tol).all(), k
        if k < 3:
            state = HN.evolve(pot, state, 0, s["mass"], ref["dt"], k * ref["output_step"], ref["output_step"], s["xmin"], s["xmax"])[0]
    assert got[0, 0].real.max() > 0
