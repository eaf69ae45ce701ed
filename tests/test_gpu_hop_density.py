"""GPU: the ensemble's phase-space density (gple_hop_bin / gple_hop_density, csrc/gple_hop.hip; DESIGN.md §17 "The ensemble in phase space") against
the numpy restatement tests/hop_density_numpy.py.

Every state is the DEVICE's own ensemble after hop_sample + hop_evolve, copied to the host: the restatement bins the same bits, so a difference
is the binning's alone.  293 trajectories (no multiple of 64 or 256), x0 = -4, sigma_p = p0 / 20, bounds +-6, mass 2000, as tests/test_gpu_hop.py.
Count planes and tallies must be EQUAL.  A coherence plane may differ by at most the count of the cell: the device's and numpy's 2^32 c_a conj(c_b)
differ by about 2^32 1e-15, far below 1/2, so each rint differs by at most one unit; the precondition that no sign convention can flip between
the two (the last non-zero component of every eigenvector column above 1e-9 at every binned x) is asserted, and no trajectory is set aside."""
import ctypes as C
import functools

import numpy as np
import pytest

from gaussian_process_liouville_equation_amd import _capi, hopping, pes, reconstruct
from tests import hop_density_numpy as HD
from tests import hop_numpy as HN

pytestmark = pytest.mark.gpu
N_TRAJ, X0, MASS, LEFT, RIGHT, SEED = 293, -4.0, 2000.0, -6.0, 6.0, 0
BAD_ARG = 1

CASES = {
    "dac16": dict(model=HN.DAC, N=2, p0=16.0, dt=1.0, steps=250),                        # all running
    "dac10": dict(model=HN.DAC, N=2, p0=10.0, dt=2.0, steps=900),                        # some have left on either side: the status mask
    "tsac": dict(model=HN.TSAC, N=3, p0=10.0, dt=4.0, steps=250, surface0=1),
    "table3": dict(model=HN.TSAC, N=3, p0=10.0, dt=4.0, steps=250, surface0=1, tabulated=True),
}
_states = {}


@functools.lru_cache(maxsize=None)
def tabulated(model, N):
    """pes.tabulate of a built-in model on [-8, 8] at dx = 1 / 16"""
    return HN.FunctionTable(*pes.tabulate(HN.scalar_function(HN.builtin(model, N)), -8.0, 1.0 / 16.0, 257))


def case_of(name):
    c = {"surface0": 0, "tabulated": False, **CASES[name]}
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


def state_of(gpu, name, model, n=N_TRAJ):
    """the device's own ensemble of the case, on the host; made once"""
    if (name, n) not in _states:
        c = case_of(name)
        start = gpu.hop_sample(c["N"], model, n, SEED, X0, c["p0"], 1.0 / (2.0 * c["p0"] / 20.0), c["p0"] / 20.0, c["surface0"])
        _states[name, n] = gpu.hop_evolve(c["N"], model, start, SEED, MASS, c["dt"], 0, c["steps"], LEFT, RIGHT)
    return _states[name, n]


def grids(name, state):
    """16 x 9 over the bounds (adds collide), 1 x 1 over everything (one address), one that leaves selected trajectories outside, 64 x 48"""
    p_first, dp = (0.0, 3.75) if name == "dac16" else (-20.0, 5.0)
    running = state[4] == 0
    return {"16x9": (LEFT, 0.8, 16, p_first, dp, 9), "1x1": (0.0, 1e3, 1, 0.0, 1e3, 1),
            "partial": (float(np.median(state[0][running])), 0.3, 7, p_first, dp, 9), "64x48": (LEFT, 12.0 / 63.0, 64, -32.0, 64.0 / 47.0, 48)}


def split(acc, N, grid):
    n_cells = grid[2] * grid[5]
    return acc[:N * n_cells].reshape(N, n_cells), acc[N * n_cells:-2].reshape(N * (N - 1), n_cells), acc[-2:]


def to_device(gpu, arrays):
    import torch

    where = torch.device("cuda", gpu.device)
    out = tuple(torch.from_numpy(np.array(a)).to(where) for a in arrays)
    torch.cuda.synchronize(where)
    return out


# ---- 1 - 3. the integers against the restatement, the density of the device's integers bit for bit ------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_against_the_restatement(gpu, model_of, name):
    c = case_of(name)
    N, model = c["N"], model_of(c)
    state = state_of(gpu, name, model)
    worst = 0
    for label, grid in grids(name, state).items():
        for bin_all in ((False, True) if name == "dac10" else (False,)):
            want = HD.bin(c["potential"], state, grid, bin_all)
            counts, coherences, tallies = split(want, N, grid)
            selected, cell = HD.cells(state, grid, bin_all)
            # the preconditions, on the restatement: the case tests something, and no sign convention can flip
            if label == "16x9":
                assert (counts.sum(axis=1) > 0).all() and counts.sum(axis=0).max() >= 2 and coherences.any(), "the case tests nothing"
            if label == "partial":
                assert tallies[0] > 0 and tallies[1] > 0, "the grid leaves nobody outside"
            assert tallies.sum() == (N_TRAJ if bin_all else (state[4] == 0).sum()) and ((state[4] != 0).any() or name != "dac10")
            Cm = HN.states(state[0][cell >= 0], c["potential"])[2]
            last = np.zeros((Cm.shape[0], N))
            for i in range(N):
                last = np.where(Cm[:, i, :] != 0, Cm[:, i, :], last)
            assert np.abs(last).min() > 1e-9
            got = gpu.hop_bin(N, model, state, grid, bin_all=bin_all)
            assert got.dtype == np.int64 and got.shape == want.shape
            g_counts, g_coherences, g_tallies = split(got, N, grid)
            assert np.array_equal(g_counts, counts) and np.array_equal(g_tallies, tallies)
            diff = np.abs(g_coherences - coherences)
            worst = max(worst, int(diff.max()))
            assert (diff <= counts.sum(axis=0)[None, :]).all()
            rho = gpu.hop_density(N, grid, got, N_TRAJ)
            ref = HD.density(got, N, grid, N_TRAJ)
            assert rho.dtype == np.complex128 and rho.shape == (N, N, grid[2], grid[5])
            assert np.array_equal(rho.view(np.float64).view(np.uint64), ref.view(np.float64).view(np.uint64))  # the signs of the zeros too
    print(f"hop bin {name}: the largest difference of a coherence sum is {worst} unit(s) of 2^-32")


# ---- 4. bits ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dac10", "table3"])
def test_bits(gpu, model_of, name):
    c = case_of(name)
    N, model = c["N"], model_of(c)
    state = state_of(gpu, name, model)
    for label, grid in grids(name, state).items():
        whole = gpu.hop_bin(N, model, state, grid, bin_all=True)
        assert np.array_equal(gpu.hop_bin(N, model, state, grid, bin_all=True), whole)                       # a repeat
        on_device = to_device(gpu, state)                                                                  # device pointers
        acc = gpu.hop_bin(N, model, on_device, grid, bin_all=True)
        rho = gpu.hop_density(N, grid, acc, N_TRAJ)
        gpu.synchronize()
        assert acc.is_cuda and rho.is_cuda and np.array_equal(acc.cpu().numpy(), whole)
        assert np.array_equal(rho.cpu().numpy().view(np.uint64), gpu.hop_density(N, grid, whole, N_TRAJ).view(np.uint64))
        part = gpu.hop_bin(N, model, tuple(a[:100] for a in state), grid, bin_all=True)                    # two slices, the second accumulated
        assert not np.array_equal(part, whole)
        assert np.array_equal(gpu.hop_bin(N, model, tuple(a[100:] for a in state), grid, acc=part, bin_all=True), whole)
        part_d = gpu.hop_bin(N, model, tuple(a[:100].contiguous() for a in on_device), grid, bin_all=True)
        both_d = gpu.hop_bin(N, model, tuple(a[100:].contiguous() for a in on_device), grid, acc=part_d, bin_all=True)
        gpu.synchronize()
        assert both_d is part_d and np.array_equal(both_d.cpu().numpy(), whole)
        dirty = np.full(len(whole), -7, dtype=np.int64)                                                    # without the flag acc is cleared first
        llp = C.POINTER(C.c_longlong)
        held = gpu._hop_state(N, state)[0]
        pointers, flags = gpu._hop_pointers(held)
        assert gpu.lib.gple_hop_bin(gpu.ctx, N, model, N_TRAJ, *grid, flags | _capi.HOP_BIN_ALL, *pointers, dirty.ctypes.data_as(llp)) == 0
        assert np.array_equal(dirty, whole)
    if name == "dac10":                                                                                    # the finished ones are the difference
        grid = grids(name, state)["1x1"]
        default, everyone = gpu.hop_bin(N, model, state, grid), gpu.hop_bin(N, model, state, grid, bin_all=True)
        assert default[-2] == (state[4] == 0).sum() < everyone[-2] == N_TRAJ


def test_one_address_against_observe(gpu):
    """65536 trajectories into the 1 x 1 grid: every count goes to one of two addresses, and the counts are hop_observe's"""
    c = case_of("dac10")
    n = 65536
    start = gpu.hop_sample(2, c["model"], n, SEED, X0, c["p0"], 1.0 / (2.0 * c["p0"] / 20.0), c["p0"] / 20.0, 0, device_out=True)
    state = gpu.hop_evolve(2, c["model"], start, SEED, MASS, c["dt"], 0, c["steps"], LEFT, RIGHT)
    counts = gpu.hop_observe(2, c["model"], state, MASS)[:6].reshape(3, 2)
    grid = (0.0, 1e3, 1, 0.0, 1e3, 1)
    running = gpu.hop_bin(2, c["model"], state, grid)
    everyone = gpu.hop_bin(2, c["model"], state, grid, bin_all=True)
    gpu.synchronize()
    running, everyone = running.cpu().numpy(), everyone.cpu().numpy()
    assert counts.sum() == n and counts[0].sum() > 0 and counts[1:].sum() > 0
    assert np.array_equal(running[:2], counts[0]) and list(running[-2:]) == [counts[0].sum(), 0]
    assert np.array_equal(everyone[:2], counts.sum(axis=0)) and list(everyone[-2:]) == [n, 0]


# ---- 5. GPLE_ERR_BAD_ARG ------------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments(gpu):
    import gaussian_process_liouville_equation_amd as pkg

    state = state_of(gpu, "dac16", HN.DAC)
    x, p, b, surface, status = (a.copy() for a in state)
    dp_, ip, llp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_longlong)
    arrays = dict(x=x.ctypes.data_as(dp_), p=p.ctypes.data_as(dp_), b=b.ctypes.data_as(dp_), surface=surface.ctypes.data_as(ip), status=status.ctypes.data_as(ip))
    acc = np.full(4 * 16 * 9 + 2, -7, dtype=np.int64)
    rho = np.full(2 * 4 * 16 * 9, -7.0)
    nan, inf = float("nan"), float("inf")
    lib, ctx = gpu.lib, gpu.ctx

    def bin_(**kw):
        a = dict(num_pes=2, model=1, n=N_TRAJ, x_first=LEFT, dx=0.8, n_x=16, p_first=0.0, dp=3.75, n_p=9, flags=0, acc=acc.ctypes.data_as(llp), **arrays)
        a.update(kw)
        return lib.gple_hop_bin(ctx, a["num_pes"], a["model"], a["n"], a["x_first"], a["dx"], a["n_x"], a["p_first"], a["dp"], a["n_p"], a["flags"], a["x"], a["p"],
                                a["b"], a["surface"], a["status"], a["acc"])

    def density(**kw):
        a = dict(num_pes=2, n_x=16, n_p=9, dx=0.8, dp=3.75, n_norm=N_TRAJ, flags=0, acc=acc.ctypes.data_as(llp), rho=rho.ctypes.data_as(dp_))
        a.update(kw)
        return lib.gple_hop_density(ctx, a["num_pes"], a["n_x"], a["n_p"], a["dx"], a["dp"], a["n_norm"], a["flags"], a["acc"], a["rho"])

    table = tabulated(HN.DAC, 2)
    mine = gpu.pes_define(2, table.x_first, table.dx, table.V, table.dV)
    other = pkg.open_api(0)
    try:
        theirs = other.pes_define(2, table.x_first, table.dx, table.V, table.dV)
        theirs = other.pes_define(2, table.x_first, table.dx, table.V, table.dV)  # a second slot, free on the session's context
        assert theirs != mine
        sizes = [dict(n_x=0), dict(n_p=0), dict(n_x=(1 << 28) + 1, n_p=1), dict(n_x=1 << 15, n_p=(1 << 13) + 1), dict(n_x=1 << 62, n_p=4), dict(n_p=1 << 63),
                 dict(dx=0.0), dict(dx=-1.0), dict(dx=nan), dict(dx=inf), dict(dp=0.0), dict(dp=-1.0), dict(dp=nan), dict(dp=inf)]
        for kw in [dict(num_pes=1), dict(num_pes=4), dict(model=-1), dict(model=3), dict(model=7), dict(model=_capi.PES_USER + 15), dict(model=theirs),
                   dict(model=mine, num_pes=3), dict(n=0), dict(n=(1 << 32) + 1), dict(x_first=nan), dict(x_first=inf), dict(p_first=nan), dict(p_first=-inf),
                   dict(acc=None)] + sizes + [{k: None} for k in arrays]:
            assert bin_(**kw) == BAD_ARG, kw
        for kw in [dict(num_pes=1), dict(num_pes=4), dict(n_norm=0), dict(acc=None), dict(rho=None)] + sizes:
            assert density(**kw) == BAD_ARG, kw
        assert (acc == -7).all() and (rho == -7.0).all()  # a refused call writes nothing
        assert bin_(model=mine) == 0 and (acc[:2 * 16 * 9] >= 0).all() and acc[-2] + acc[-1] == N_TRAJ and density() == 0 and np.isfinite(rho).all()
    finally:
        other.close()
        gpu.pes_undefine(mine)


# ---- 6. the driver, and the directory it writes under reconstruct.run_files ---------------------------------------------------------------------------
def test_driver_and_the_reconstruction_of_its_directory(gpu, tmp_path):
    kw = dict(model=hopping.DAC, num_pes=2, ln_energy=-2.0, n_traj=512, seed=SEED, dt=2.0, x0=X0, xmin=LEFT, xmax=RIGHT, phase_grid=(32, 24), max_outputs=3,
              output_time=200.0)  # t = 0, 200, 400: the packet reaches the crossings, both surfaces and the coherences fill
    res = hopping.run(gpu, out_dir=str(tmp_path / "device"), **kw)
    ref = hopping.run(HD.NumpyHopDensityApi(), out_dir=str(tmp_path / "numpy"), **kw)
    assert len(res["records"]) == len(ref["records"]) == 3 and res["state"][0].is_cuda
    x, p = (reconstruct.read_grid(tmp_path / "device" / name) for name in ("x.txt", "p.txt"))
    assert len(x) == 32 and len(p) == 24
    for name in ("x.txt", "p.txt", "t.txt"):
        assert (tmp_path / "device" / name).read_text() == (tmp_path / "numpy" / name).read_text()
    unit = 1.0 / (512 * (12.0 / 31.0) * (p[1] - p[0]))  # the density of one trajectory in a cell
    blocks = [list(reconstruct.phase_blocks(str(tmp_path / d / "phase.txt"), 2, 32, 24)) for d in ("device", "numpy")]
    assert len(blocks[0]) == len(blocks[1]) == 3
    for a, b, got, want in zip(res["records"], ref["records"], *blocks):
        running = int(a["counts"][hopping.RUNNING].sum())
        assert a["t"] == b["t"] and (a["binned"], a["outside"]) == (b["binned"], b["outside"]) == (running, 0) and running > 0
        assert np.array_equal(a["binned_counts"], b["binned_counts"]) and np.array_equal(a["binned_counts"], a["counts"][hopping.RUNNING])
        got, want = (reconstruct._parse_host(block)[0].view(np.complex128).reshape(2, 2, 32, 24) for block in (got, want))
        # "%g" on either side: 5e-6 of the value each; the integers: one unit of 2^-32 per trajectory of the cell
        count = np.rint((want[0, 0].real + want[1, 1].real) / unit)
        assert count.sum() == running
        tol = 1.1e-5 * np.abs(want) + (count + 1.0)[None, None] * unit / 4294967296.0
        assert (np.abs(got.real - want.real) <= tol).all() and (np.abs(got.imag - want.imag) <= tol).all()
    assert np.abs(got[0, 1]).max() > 0  # coherences were written
    # the pipeline: the GP of reconstruct on the histogram (the accuracy of a fit to 512 trajectories is not asserted)
    # n_points = 8: grid_select draws among the cells that hold something, and the sparsest plane that is fitted (rho_11 at t = 200) has 9
    recs = reconstruct.run_files(gpu, str(tmp_path / "device"), out_dir=str(tmp_path / "recon"), model=hopping.DAC, num_pes=2, mass=MASS, n_points=8, maxeval=60, seed=11)
    assert [r["index"] for r in recs] == [0, 1, 2]
    for r, rec in zip(recs, res["records"]):
        for key in ("nlml", "hyper", "mse_before", "mse_after", "population_exact", "population_gpr_after"):
            assert np.isfinite(r[key]).all(), key
        # the grid's own sum is the fraction binned, in the cell size run_files takes from the reference, (x[nx - 1] - x[0]) / nx (main_evolve.cpp:23)
        assert abs(r["population_exact"].sum() - rec["binned"] / 512 * (31.0 / 32.0) * (23.0 / 24.0)) < 1e-4
