"""GPU: the ensemble's phase-space density from the amplitudes (gple_hop_bin_mf / gple_hop_density_mf, csrc/gple_hop.hip; DESIGN.md §17 "The
ensemble in phase space, from the amplitudes") against the numpy restatement tests/hop_density_mf_numpy.py and against gple_hop_bin itself.

Every state is the DEVICE's own ensemble after hop_sample + hop_evolve_mf (one case: hop_evolve), copied to the host: the restatement bins the
same bits, so a difference is the binning's alone.  293 trajectories, seed 0 (a ragged last wave and a ragged last block), x0 = -4,
sigma_p = p0 / 20, bounds +-6, mass 2000.  The tallies must be EQUAL.  A weight or a coherence sum may differ by at most the count of its cell:
the device's and numpy's 2^32 c_a conj(c_b) differ by about 2^32 1e-15, far below 1/2, so each rint differs by at most one unit.  For the
coherence planes the precondition that no sign convention can flip between the two (the last non-zero component of every eigenvector column
above 1e-9 at every binned x) is asserted; a weight |c_a|^2 does not see the sign.  No trajectory is set aside."""
import ctypes as C
import functools

import numpy as np
import pytest

from gaussian_process_liouville_equation_amd import _capi, hopping, pes, reconstruct
from tests import hop_density_mf_numpy as HDM
from tests import hop_numpy as HN

pytestmark = pytest.mark.gpu
N_TRAJ, X0, MASS, LEFT, RIGHT, SEED = 293, -4.0, 2000.0, -6.0, 6.0, 0
BAD_ARG = 1
TWO32 = 4294967296

CASES = {
    "dac16": dict(model=HN.DAC, N=2, p0=16.0, dt=1.0, steps=250),                        # all running
    "dac10": dict(model=HN.DAC, N=2, p0=10.0, dt=2.0, steps=900),                        # all three statuses
    "tsac": dict(model=HN.TSAC, N=3, p0=10.0, dt=4.0, steps=400, surface0=1),
    "table2": dict(model=HN.DAC, N=2, p0=10.0, dt=2.0, steps=900, tabulated=True),
    "fssh": dict(model=HN.DAC, N=2, p0=10.0, dt=2.0, steps=900, hops=True),              # a fewest-switches ensemble: the other prescription
}
_states = {}


@functools.lru_cache(maxsize=None)
def tabulated(model, N):
    """pes.tabulate of a built-in model on [-8, 8] at dx = 1 / 16"""
    return HN.FunctionTable(*pes.tabulate(HN.scalar_function(HN.builtin(model, N)), -8.0, 1.0 / 16.0, 257))


def case_of(name):
    c = {"surface0": 0, "tabulated": False, "hops": False, **CASES[name]}
    c["potential"] = HN.table(tabulated(c["model"], c["N"])) if c["tabulated"] else HN.builtin(c["model"], c["N"])
    return c


@pytest.fixture
def model_of(gpu):
    ids = []

    def make(c):
        if not c["tabulated"]:
            return c["model"]
        t = tabulated(c["model"], c["N"])
        ids.append(gpu.pes_define(c["N"], t.x_first, t.dx, t.V, t.dV))
        return ids[-1]

    yield make
    for model in ids:
        gpu.pes_undefine(model)


def sample_of(gpu, c, model, n=N_TRAJ, **kw):
    return gpu.hop_sample(c["N"], model, n, SEED, X0, c["p0"], 1.0 / (2.0 * c["p0"] / 20.0), c["p0"] / 20.0, c["surface0"], **kw)


def evolved(gpu, c, model, start):
    if c["hops"]:
        return gpu.hop_evolve(c["N"], model, start, SEED, MASS, c["dt"], 0, c["steps"], LEFT, RIGHT)
    return gpu.hop_evolve_mf(c["N"], model, start, MASS, c["dt"], c["steps"], LEFT, RIGHT)


def state_of(gpu, name, model):
    """the device's own ensemble of the case, on the host; made once"""
    if name not in _states:
        c = case_of(name)
        _states[name] = evolved(gpu, c, model, sample_of(gpu, c, model))
    return _states[name]


def grids(name, state):
    """16 x 9 over the bounds (adds collide), 1 x 1 over everything (one address), one that leaves selected trajectories outside, 64 x 48"""
    p_first, dp = (0.0, 3.75) if name == "dac16" else (-20.0, 5.0)
    running = state[4] == 0
    return {"16x9": (LEFT, 0.8, 16, p_first, dp, 9), "1x1": (0.0, 1e3, 1, 0.0, 1e3, 1),
            "partial": (float(np.median(state[0][running])), 0.3, 7, p_first, dp, 9), "64x48": (LEFT, 12.0 / 63.0, 64, -32.0, 64.0 / 47.0, 48)}


def split(acc, N, grid):
    n_cells = grid[2] * grid[5]
    return acc[:N * n_cells].reshape(N, n_cells), acc[N * n_cells:-2].reshape(N * (N - 1), n_cells), acc[-2:]


def counts_of(state, grid, bin_all):
    """the selected trajectories per cell"""
    _, cell = HDM.cells(state, grid, bin_all)
    return np.bincount(cell[cell >= 0], minlength=grid[2] * grid[5])


def to_device(gpu, arrays):
    import torch

    where = torch.device("cuda", gpu.device)
    out = tuple(torch.from_numpy(np.array(a)).to(where) for a in arrays)
    torch.cuda.synchronize(where)
    return out


def flags_of(name, state):
    return (False, True) if (state[4] != 0).any() else (False,)


# ---- 1. the integers against the restatement, the density of the device's integers bit for bit ---------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_against_the_restatement(gpu, model_of, name):
    c = case_of(name)
    N, model = c["N"], model_of(c)
    state = state_of(gpu, name, model)
    assert name not in ("dac10", "table2", "fssh") or all((state[4] == s).any() for s in (0, 1, 2))
    worst = [0, 0]
    for label, grid in grids(name, state).items():
        for bin_all in flags_of(name, state):
            want = HDM.bin_mf(c["potential"], state, grid, bin_all)
            weights, coherences, tallies = split(want, N, grid)
            count = counts_of(state, grid, bin_all)
            selected, cell = HDM.cells(state, grid, bin_all)
            # the preconditions, on the restatement: the case tests something, and no sign convention can flip
            if label == "16x9":
                assert (weights.sum(axis=1) > TWO32).all() and count.max() >= 2 and coherences.any(), "the case tests nothing"
            if label == "partial":
                assert tallies[0] > 0 and tallies[1] > 0, "the grid leaves nobody outside"
            assert count.sum() == tallies[0] and tallies.sum() == (N_TRAJ if bin_all else (state[4] == 0).sum())
            Cm = HN.states(state[0][cell >= 0], c["potential"])[2]
            last = np.zeros((Cm.shape[0], N))
            for i in range(N):
                last = np.where(Cm[:, i, :] != 0, Cm[:, i, :], last)
            assert np.abs(last).min() > 1e-9
            got = gpu.hop_bin_mf(N, model, state, grid, bin_all=bin_all)
            assert got.dtype == np.int64 and got.shape == want.shape
            g_weights, g_coherences, g_tallies = split(got, N, grid)
            assert np.array_equal(g_tallies, tallies)
            d_w, d_c = np.abs(g_weights - weights), np.abs(g_coherences - coherences)
            worst = [max(worst[0], int(d_w.max())), max(worst[1], int(d_c.max()))]
            assert (d_w <= count[None, :]).all() and (d_c <= count[None, :]).all()
            rho = gpu.hop_density_mf(N, grid, got, N_TRAJ)
            ref = HDM.density_mf(got, N, grid, N_TRAJ)
            assert rho.dtype == np.complex128 and rho.shape == (N, N, grid[2], grid[5])
            assert np.array_equal(rho.view(np.float64).view(np.uint64), ref.view(np.float64).view(np.uint64))  # the signs of the zeros too
    print(f"hop bin_mf {name}: the largest difference of a weight sum is {worst[0]}, of a coherence sum {worst[1]} unit(s) of 2^-32")


# ---- 2. device against device: gple_hop_bin on the same state and flags -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_against_the_mixed_density(gpu, model_of, name):
    """the surface of every ensemble here is in range (a mean-field step hands it through), so gple_hop_bin selects the same trajectories"""
    c = case_of(name)
    N, model = c["N"], model_of(c)
    state = state_of(gpu, name, model)
    assert ((state[3] >= 0) & (state[3] < N)).all()
    worst = [0, 0]
    for label, grid in grids(name, state).items():
        for bin_all in flags_of(name, state):
            mixed, mf = gpu.hop_bin(N, model, state, grid, bin_all=bin_all), gpu.hop_bin_mf(N, model, state, grid, bin_all=bin_all)
            counts, coherences, tallies = split(mixed, N, grid)
            weights, mf_coherences, mf_tallies = split(mf, N, grid)
            count = counts.sum(axis=0)
            assert np.array_equal(mf_tallies, tallies) and count.sum() == tallies[0]
            d_c = np.abs(mf_coherences - coherences)
            off = np.abs(weights.sum(axis=0) - TWO32 * count)
            worst = [max(worst[0], int(d_c.max())), max(worst[1], int(off.max()))]
            assert (d_c <= count[None, :]).all()
            assert (off <= count * (N / 2.0 + 1.0)).all()
    print(f"hop bin_mf against hop_bin {name}: coherence sums differ by at most {worst[0]}, a cell's weights are off its count by at most {worst[1]} unit(s)")
    start = sample_of(gpu, c, model)  # t = 0: a weight is exactly 2^32 per trajectory of the surface
    for label, grid in grids(name, start).items():
        mixed, mf = gpu.hop_bin(N, model, start, grid), gpu.hop_bin_mf(N, model, start, grid)
        n_cells = grid[2] * grid[5]
        assert mixed[-2] > 0 and np.array_equal(mf[:N * n_cells], TWO32 * mixed[:N * n_cells]) and np.array_equal(mf[N * n_cells:], mixed[N * n_cells:])


# ---- 3. bits --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dac10", "tsac", "table2"])
def test_bits(gpu, model_of, name):
    c = case_of(name)
    N, model = c["N"], model_of(c)
    state = state_of(gpu, name, model)
    llp = C.POINTER(C.c_longlong)
    for label, grid in grids(name, state).items():
        whole = gpu.hop_bin_mf(N, model, state, grid, bin_all=True)
        assert np.array_equal(gpu.hop_bin_mf(N, model, state, grid, bin_all=True), whole)                    # a repeat
        on_device = to_device(gpu, state)                                                                  # device pointers
        acc = gpu.hop_bin_mf(N, model, on_device, grid, bin_all=True)
        rho = gpu.hop_density_mf(N, grid, acc, N_TRAJ)
        gpu.synchronize()
        assert acc.is_cuda and rho.is_cuda and np.array_equal(acc.cpu().numpy(), whole)
        assert np.array_equal(rho.cpu().numpy().view(np.uint64), gpu.hop_density_mf(N, grid, whole, N_TRAJ).view(np.uint64))
        part = gpu.hop_bin_mf(N, model, tuple(a[:100] for a in state), grid, bin_all=True)                 # two slices, the second accumulated
        assert not np.array_equal(part, whole)
        assert np.array_equal(gpu.hop_bin_mf(N, model, tuple(a[100:] for a in state), grid, acc=part, bin_all=True), whole)
        part_d = gpu.hop_bin_mf(N, model, tuple(a[:100].contiguous() for a in on_device), grid, bin_all=True)
        both_d = gpu.hop_bin_mf(N, model, tuple(a[100:].contiguous() for a in on_device), grid, acc=part_d, bin_all=True)
        gpu.synchronize()
        assert both_d is part_d and np.array_equal(both_d.cpu().numpy(), whole)
        dirty = np.full(len(whole), -7, dtype=np.int64)                                                    # without the flag acc is cleared first
        held = gpu._hop_mf_state(N, state, False)[0]
        pointers, flags = gpu._hop_mf_pointers(held)
        assert gpu.lib.gple_hop_bin_mf(gpu.ctx, N, model, N_TRAJ, *grid, flags | _capi.HOP_BIN_ALL, *pointers, dirty.ctypes.data_as(llp)) == 0
        assert np.array_equal(dirty, whole)
        order = np.random.default_rng(5).permutation(N_TRAJ)                                               # a permuted ensemble
        assert np.array_equal(gpu.hop_bin_mf(N, model, tuple(np.ascontiguousarray(a[order]) for a in state), grid, bin_all=True), whole)
        odd = (state[0], state[1], state[2], np.full(N_TRAJ, 7, dtype=np.int32), state[4])                 # the surface is not read
        assert np.array_equal(gpu.hop_bin_mf(N, model, odd, grid, bin_all=True), whole)
    if name != "tsac":                                                                                     # the finished ones are the difference
        grid = grids(name, state)["1x1"]
        default, everyone = gpu.hop_bin_mf(N, model, state, grid), gpu.hop_bin_mf(N, model, state, grid, bin_all=True)
        assert default[-2] == (state[4] == 0).sum() < everyone[-2] == N_TRAJ and (default[:N] < everyone[:N]).all()


def test_one_address_against_observe_mf(gpu):
    """65536 trajectories into the 1 x 1 grid: every weight goes to one of two addresses, and the sums are hop_observe_mf's, within the n
    roundings of half a unit and the rounding of the tree sums (1e-12 n)"""
    c = case_of("dac10")
    n = 65536
    state = evolved(gpu, c, c["model"], sample_of(gpu, c, c["model"], n, device_out=True))
    sums = gpu.hop_observe_mf(2, c["model"], state, MASS)
    weights, n_status = sums[:6].reshape(3, 2), sums[6:9]
    grid = (0.0, 1e3, 1, 0.0, 1e3, 1)
    running = gpu.hop_bin_mf(2, c["model"], state, grid)
    everyone = gpu.hop_bin_mf(2, c["model"], state, grid, bin_all=True)
    gpu.synchronize()
    running, everyone = running.cpu().numpy(), everyone.cpu().numpy()
    assert n_status.sum() == n and n_status[0] > 0 and n_status[1:].sum() > 0
    assert list(running[-2:]) == [n_status[0], 0] and list(everyone[-2:]) == [n, 0]
    bound = n / (2.0 * TWO32) + 1e-12 * n
    assert (np.abs(running[:2] / TWO32 - weights[0]) <= bound).all() and (np.abs(everyone[:2] / TWO32 - weights.sum(axis=0)) <= bound).all()


# ---- 4. GPLE_ERR_BAD_ARG ----------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments(gpu):
    import gaussian_process_liouville_equation_amd as pkg

    state = state_of(gpu, "dac16", HN.DAC)
    x, p, b, _, status = (a.copy() for a in state)
    dp_, ip, llp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_longlong)
    arrays = dict(x=x.ctypes.data_as(dp_), p=p.ctypes.data_as(dp_), b=b.ctypes.data_as(dp_), status=status.ctypes.data_as(ip))
    acc = np.full(4 * 16 * 9 + 2, -7, dtype=np.int64)
    rho = np.full(2 * 4 * 16 * 9, -7.0)
    nan, inf = float("nan"), float("inf")
    lib, ctx = gpu.lib, gpu.ctx

    def bin_(**kw):
        a = dict(num_pes=2, model=1, n=N_TRAJ, x_first=LEFT, dx=0.8, n_x=16, p_first=0.0, dp=3.75, n_p=9, flags=0, acc=acc.ctypes.data_as(llp), **arrays)
        a.update(kw)
        return lib.gple_hop_bin_mf(ctx, a["num_pes"], a["model"], a["n"], a["x_first"], a["dx"], a["n_x"], a["p_first"], a["dp"], a["n_p"], a["flags"], a["x"],
                                   a["p"], a["b"], a["status"], a["acc"])

    def density(**kw):
        a = dict(num_pes=2, n_x=16, n_p=9, dx=0.8, dp=3.75, n_norm=N_TRAJ, flags=0, acc=acc.ctypes.data_as(llp), rho=rho.ctypes.data_as(dp_))
        a.update(kw)
        return lib.gple_hop_density_mf(ctx, a["num_pes"], a["n_x"], a["n_p"], a["dx"], a["dp"], a["n_norm"], a["flags"], a["acc"], a["rho"])

    table = tabulated(HN.DAC, 2)
    mine = gpu.pes_define(2, table.x_first, table.dx, table.V, table.dV)
    other = pkg.open_api(0)
    try:
        theirs = other.pes_define(2, table.x_first, table.dx, table.V, table.dV)
        theirs = other.pes_define(2, table.x_first, table.dx, table.V, table.dV)  # a second slot, free on the session's context
        assert theirs != mine
        sizes = [dict(n_x=0), dict(n_p=0), dict(n_x=(1 << 28) + 1, n_p=1), dict(n_x=1 << 15, n_p=(1 << 13) + 1), dict(n_x=1 << 62, n_p=4), dict(n_p=1 << 63),
                 dict(dx=0.0), dict(dx=-1.0), dict(dx=nan), dict(dx=inf), dict(dp=0.0), dict(dp=-1.0), dict(dp=nan), dict(dp=inf)]
        # n > 2^31: the size alone, the call returns before it touches an array
        for kw in [dict(num_pes=1), dict(num_pes=4), dict(model=-1), dict(model=3), dict(model=7), dict(model=_capi.PES_USER + 15), dict(model=theirs),
                   dict(model=mine, num_pes=3), dict(n=0), dict(n=(1 << 31) + 1), dict(n=1 << 32), dict(n=(1 << 32) + 1), dict(x_first=nan), dict(x_first=inf),
                   dict(p_first=nan), dict(p_first=-inf), dict(acc=None)] + sizes + [{k: None} for k in arrays]:
            assert bin_(**kw) == BAD_ARG, kw
        for kw in [dict(num_pes=1), dict(num_pes=4), dict(n_norm=0), dict(acc=None), dict(rho=None)] + sizes:
            assert density(**kw) == BAD_ARG, kw
        assert (acc == -7).all() and (rho == -7.0).all()  # a refused call writes nothing
        assert bin_(model=mine) == 0 and (acc[:2 * 16 * 9] >= 0).all() and acc[-2] + acc[-1] == N_TRAJ and density() == 0 and np.isfinite(rho).all()
    finally:
        other.close()
        gpu.pes_undefine(mine)


# ---- 5. the timer -------------------------------------------------------------------------------------------------------------------------------------
def test_the_timer_counts_the_calls(gpu):
    state = state_of(gpu, "dac16", HN.DAC)
    gpu.enable_timing(True)
    try:
        before = gpu.timing(_capi.TIMER_HOP_BIN_MF)[2], gpu.timing(_capi.TIMER_HOP_BIN)[2]
        gpu.hop_bin_mf(2, HN.DAC, state, (LEFT, 0.8, 16, 0.0, 3.75, 9))
        last, _, count = gpu.timing(_capi.TIMER_HOP_BIN_MF)
        assert count == before[0] + 1 and last > 0.0 and gpu.timing(_capi.TIMER_HOP_BIN)[2] == before[1]
    finally:
        gpu.enable_timing(False)


# ---- 6. the driver, and the directory it writes under reconstruct.run_files -----------------------------------------------------------------------
def test_driver_and_the_reconstruction_of_its_directory(gpu, tmp_path):
    kw = dict(model=hopping.DAC, num_pes=2, ln_energy=-2.0, n_traj=512, seed=SEED, dt=2.0, x0=X0, xmin=LEFT, xmax=RIGHT, phase_grid=(32, 24), max_outputs=3,
              output_time=200.0, method="ehrenfest", phase_density="amplitude")  # t = 0, 200, 400: the packet reaches the crossings
    res = hopping.run(gpu, out_dir=str(tmp_path / "device"), **kw)
    ref = hopping.run(HDM.NumpyHopDensityMfApi(), out_dir=str(tmp_path / "numpy"), **kw)
    assert len(res["records"]) == len(ref["records"]) == 3 and res["state"][0].is_cuda
    x, p = (reconstruct.read_grid(tmp_path / "device" / name) for name in ("x.txt", "p.txt"))
    assert len(x) == 32 and len(p) == 24
    for name in ("x.txt", "p.txt", "t.txt"):
        assert (tmp_path / "device" / name).read_text() == (tmp_path / "numpy" / name).read_text()
    unit = 1.0 / (512 * (12.0 / 31.0) * (p[1] - p[0]))  # the density of one trajectory in a cell
    blocks = [list(reconstruct.phase_blocks(str(tmp_path / d / "phase.txt"), 2, 32, 24)) for d in ("device", "numpy")]
    assert len(blocks[0]) == len(blocks[1]) == 3
    for a, b, got, want in zip(res["records"], ref["records"], *blocks):
        running = int(a["n_status"][hopping.RUNNING])
        assert a["t"] == b["t"] and (a["binned"], a["outside"]) == (b["binned"], b["outside"]) == (running, 0) and running > 0
        assert "binned_counts" not in a and a["binned_weights"].shape == (2,)
        assert (np.abs(a["binned_weights"] - b["binned_weights"]) <= running / TWO32).all()
        assert (np.abs(a["binned_weights"] - a["weights"][hopping.RUNNING]) <= running / (2.0 * TWO32) + 1e-12 * running).all()
        got, want = (reconstruct._parse_host(block)[0].view(np.complex128).reshape(2, 2, 32, 24) for block in (got, want))
        # "%g" on either side: 5e-6 of the value each; the integers: one unit of 2^-32 per trajectory of the cell
        count = np.rint((want[0, 0].real + want[1, 1].real) / unit)
        assert count.sum() == running
        tol = 1.1e-5 * np.abs(want) + (count + 1.0)[None, None] * unit / 4294967296.0
        assert (np.abs(got.real - want.real) <= tol).all() and (np.abs(got.imag - want.imag) <= tol).all()
    assert np.abs(got[0, 1]).max() > 0 and got[1, 1].real.max() > 0  # coherences and the upper population were written
    # the pipeline: the GP of reconstruct on the histogram (the accuracy of a fit to 512 trajectories is not asserted)
    recs = reconstruct.run_files(gpu, str(tmp_path / "device"), out_dir=str(tmp_path / "recon"), model=hopping.DAC, num_pes=2, mass=MASS, n_points=8, maxeval=60, seed=11)
    assert [r["index"] for r in recs] == [0, 1, 2]
    for r in recs:
        for key in ("nlml", "hyper", "mse_before", "mse_after", "population_exact", "population_gpr_after"):
            assert np.isfinite(r[key]).all(), key
