"""GPU: the coupled-channel scattering solver (gple_scatter, csrc/gple_scatter.hip) against the numpy restatement
tests/scatter_numpy.py, entry by entry.

Cases: SAC, DAC and ECR on [-40, 40], TSAC and tables of DAC and TSAC (dx = 1 / 16) on [-30, 30], all with N = 1500 steps, mass 2000 and the
energies of n momenta uniform in [3, 30] on the lowest surface of the left end, n = 1, 70 (a full wave and six lanes) and 257: SAC and DAC
straddle the upper threshold inside one wave.  Every entry of prob (all incoming surfaces) lies within 64 D + 1e-13 of the float64 restatement,
D being the largest distance between the float64 and the long double restatement for that case, measured here; NaN columns sit where the
restatement has them and closed final channels are exactly 0.  An energy is set aside only where the restatement's own |u_j| - 2 is within 1e-9 of
zero, and none may be.  The closed forms of tests/scatter_cases.py run on the device through tables at dx = 1 / 64 with N = 4000; the bound is
twice the long double restatement's own distance from the closed form on that table plus the tolerance above.  Small grids, in the same pattern:
the smallest grid accepted (N = 2), 3 and 5, and the grids on which the N + 1 nodes cross a block of the table kernel (255, 256, 257), SAC and
a DAC table, with n = 1, 64, 65 and 70 energies.  The ratios measured on the MI355X are in DESIGN.md §18."""
import ctypes as C
import functools

import numpy as np
import pytest

from gaussian_process_liouville_equation_amd import _capi, pes, scattering
from tests import hop_numpy as HN
from tests import scatter_cases as SC
from tests import scatter_numpy as SN

pytestmark = pytest.mark.gpu
MASS, N_STEPS = SC.MASS, 1500
BAD_ARG = 1
SIZES = (1, 70, 257)

# name: model (an id, or the built-in that is tabulated at dx = 1 / 16 on the box), levels, the box
CASES = {
    "sac": dict(model=HN.SAC, N=2, box=40.0),
    "dac": dict(model=HN.DAC, N=2, box=40.0),
    "ecr": dict(model=HN.ECR, N=2, box=40.0),
    "tsac": dict(model=HN.TSAC, N=3, box=30.0),
    "table2": dict(model=HN.DAC, N=2, box=30.0, tabulated=True),
    "table3": dict(model=HN.TSAC, N=3, box=30.0, tabulated=True),
}
CLOSED = {"eckart": SC.eckart, "rotated": SC.rotated}


@functools.lru_cache(maxsize=None)
def tabulated(model, N):
    """pes.tabulate of a built-in model on [-30, 30] at dx = 1 / 16"""
    return HN.FunctionTable(*pes.tabulate(HN.scalar_function(HN.builtin(model, N)), -30.0, 1.0 / 16.0, 961))


@functools.lru_cache(maxsize=None)
def closed_table(name):
    """pes.tabulate of a closed-form case on [-20, 20] at dx = 1 / 64"""
    return HN.FunctionTable(*pes.tabulate(SC.scalar(CLOSED[name]), -SC.BOX, 1.0 / 64.0, 2561))


@functools.lru_cache(maxsize=None)
def reference(name, n, box=None, n_steps=N_STEPS, p_max=30.0):
    """The case on the restatement, once: float64 and long double, and D.  box, n_steps, p_max: another box, grid and largest momentum than
    the case's own (the small grids)"""
    assert np.finfo(np.longdouble).eps < 1e-18  # or D calibrates nothing
    c = {"tabulated": False, **CASES[name]}
    if box is not None:
        c["box"] = box
    pot = HN.table(tabulated(c["model"], c["N"])) if c["tabulated"] else HN.builtin(c["model"], c["N"])
    eps = HN.jacobi(pot(np.array([-c["box"]]))[0])[0][0]
    p = np.linspace(3.0, p_max, n)
    energies = p * p / 2.0 / MASS + eps[0]
    ref = SN.march(pot, c["N"], MASS, -c["box"], c["box"], n_steps, energies)
    wide = SN.march(pot, c["N"], MASS, -c["box"], c["box"], n_steps, energies, dtype=np.longdouble)
    assert np.array_equal(np.isnan(ref["prob"]), np.isnan(wide["prob"]))
    D = float(np.nanmax(np.abs((ref["prob"] - wide["prob"]).astype(np.float64))))
    closed_final = np.stack([~(np.abs(ref["u_left"]) < 2.0), ~(np.abs(ref["u_right"]) < 2.0)], axis=1)  # (n, side, final surface)
    return dict(case=c, energies=energies, prob=ref["prob"], defect=ref["defect"], D=D, aside=SN.near_threshold(ref), closed_final=closed_final)


@pytest.fixture
def model_of(gpu):
    """model_of(table or id) -> the id on the session's context (a table is defined, and undefined when the test ends)"""
    ids = []

    def make(t):
        if isinstance(t, int):
            return t
        ids.append(gpu.pes_define(t.num_pes, t.x_first, t.dx, t.V, t.dV))
        return ids[-1]

    yield make
    for model in ids:
        gpu.pes_undefine(model)


def case_model(model_of, c):
    return model_of(tabulated(c["model"], c["N"]) if c["tabulated"] else c["model"])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- 1. against the restatement, and the defect ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_against_the_restatement(gpu, model_of, name):
    for n in SIZES:
        ref = reference(name, n)
        c = ref["case"]
        prob, defect = gpu.scatter(c["N"], case_model(model_of, c), MASS, -c["box"], c["box"], N_STEPS, ref["energies"])
        assert ref["aside"].sum() <= 0
        closed_in = np.isnan(ref["prob"])
        assert np.array_equal(np.isnan(prob), closed_in) and np.array_equal(np.isnan(defect), np.isnan(ref["defect"]))
        exact_zero = np.broadcast_to(ref["closed_final"][:, None], prob.shape) & ~closed_in
        assert (prob[exact_zero] == 0.0).all() and (ref["prob"][exact_zero] == 0.0).all()
        tol = 64.0 * ref["D"] + 1e-13
        err = float(np.nanmax(np.abs(prob - ref["prob"])))
        open_defect = float(np.nanmax(np.abs(defect)))
        print(f"scatter parity {name} n = {n}: closed incoming columns {int(np.isnan(ref['defect']).sum())}, closed final entries {int(exact_zero.sum())}, "
              f"D {ref['D']:.3g}, err / tol {err / tol:.3g}, largest |defect| {open_defect:.3g}")
        if n == 257 and name != "ecr":  # (ECR's upper surface is open at the left for every momentum here; it is closed at the right below p = 28.3)
            top = np.isnan(ref["defect"][:, -1])
            flips = np.nonzero(top[1:] != top[:-1])[0]
            assert len(flips) and (flips // 64 == (flips + 1) // 64).all(), "no threshold inside a wave: the case tests less than it says"
        assert err <= tol, (name, n, err, tol)
        assert open_defect < 1e-11


# ---- 1b. small grids: the march reads V_n one step ahead and the table kernel runs (n_steps + 256) / 256 blocks of 256 ------------------------------------------
# name, box, n_steps, the largest momentum: the smallest grid gple_scatter accepts (2) and 3, an odd small one, and the grids on which
# n_steps + 1 nodes fill a block but for one, exactly, and with one over.  The largest momentum keeps c (E_max - eps_min) below 1 / 2: a grid
# without an open discrete channel is refused (BAD_ARG), and the restatement does not refuse
SMALL_GRIDS = [("sac", 0.25, 2, 9.0), ("sac", 0.25, 3, 14.0), ("sac", 1.0, 5, 6.0), ("sac", 10.0, 255, 30.0), ("sac", 10.0, 256, 30.0), ("sac", 10.0, 257, 30.0),
               ("table2", 10.0, 255, 30.0), ("table2", 10.0, 256, 30.0)]
SMALL_SIZES = (1, 64, 65, 70)  # one energy, a full wave, a wave and one lane, a wave and six: exact and ragged last waves of the one-wave workgroups


@pytest.mark.parametrize("name, box, n_steps, p_max", SMALL_GRIDS, ids=[f"{name}-{box:g}-{n_steps}" for name, box, n_steps, _ in SMALL_GRIDS])
def test_small_grids_against_the_restatement(gpu, model_of, name, box, n_steps, p_max):
    c = reference(name, SMALL_SIZES[0], box, n_steps, p_max)["case"]
    model = case_model(model_of, c)
    for n in SMALL_SIZES:
        ref = reference(name, n, box, n_steps, p_max)
        prob, defect = gpu.scatter(c["N"], model, MASS, -box, box, n_steps, ref["energies"])
        again = gpu.scatter(c["N"], model, MASS, -box, box, n_steps, ref["energies"])
        assert ref["aside"].sum() <= 0  # near_threshold sets nothing aside
        closed_in = np.isnan(ref["prob"])
        assert np.array_equal(np.isnan(prob), closed_in) and np.array_equal(np.isnan(defect), np.isnan(ref["defect"]))
        exact_zero = np.broadcast_to(ref["closed_final"][:, None], prob.shape) & ~closed_in
        assert (prob[exact_zero] == 0.0).all() and (ref["prob"][exact_zero] == 0.0).all()
        tol = 64.0 * ref["D"] + 1e-13
        err = float(np.nanmax(np.abs(prob - ref["prob"])))
        open_defect = float(np.nanmax(np.abs(defect)))
        T00 = ref["prob"][:, 0, 1, 0]
        print(f"scatter small grid {name} box {box:g} N = {n_steps} n = {n}: closed incoming columns {int(np.isnan(ref['defect']).sum())}, closed final entries "
              f"{int(exact_zero.sum())}, T00 {T00.min():.3g} ... {T00.max():.3g}, D {ref['D']:.3g}, err / tol {err / tol:.3g}, largest |defect| {open_defect:.3g}")
        assert np.isfinite(T00).all()  # the lowest surface is open at every energy: no case is hollow
        assert err <= tol, (name, box, n_steps, n, err, tol)
        assert open_defect < 1e-11
        assert same_bits(again[0], prob) and same_bits(again[1], defect)  # a repeat


# ---- 2. closed forms on the device -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CLOSED))
def test_closed_forms_on_the_device(gpu, model_of, name):
    tab = closed_table(name)
    pot = HN.table(tab)
    args = (2, MASS, -SC.BOX, SC.BOX, 4000, [SC.E_IN])
    ref, wide = SN.march(pot, *args), SN.march(pot, *args, dtype=np.longdouble)
    tol = 64.0 * float(np.abs((ref["prob"] - wide["prob"]).astype(np.float64)).max()) + 1e-13
    prob, _ = gpu.scatter(2, model_of(tab), MASS, -SC.BOX, SC.BOX, 4000, [SC.E_IN])
    exact = SC.closed_forms()[name]
    channels = [(0, exact)] if name == "eckart" else [(0, exact[0]), (1, exact[1])]
    for k, T in channels:
        own = float(abs(wide["prob"][0, k, 1, k] - T))
        got = float(abs(np.longdouble(prob[0, k, 1, k]) - T))
        print(f"scatter closed form {name} channel {k}: T {float(T):.11f}, long double restatement on the table off by {own:.3g}, device off by {got:.3g}, "
              f"bound {2.0 * own + tol:.3g}")
        assert got <= 2.0 * own + tol
    assert float(np.abs(prob - ref["prob"]).max()) <= tol


# ---- 3. bits -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dac", "table3"])
def test_bits(gpu, model_of, name):
    import torch

    ref = reference(name, 257)
    c = ref["case"]
    model = case_model(model_of, c)
    call = lambda energies, **kw: gpu.scatter(c["N"], model, MASS, -c["box"], c["box"], N_STEPS, energies, **kw)
    prob, defect = call(ref["energies"])
    again = call(ref["energies"])
    assert same_bits(again[0], prob) and same_bits(again[1], defect)                     # a repeat
    alone, none = call(ref["energies"], want_defect=False)                               # defect = NULL
    assert none is None and same_bits(alone, prob)
    where = torch.device("cuda", gpu.device)                                             # device pointers
    on_device = call(torch.from_numpy(ref["energies"].copy()).to(where))
    assert on_device[0].is_cuda and on_device[1].is_cuda
    assert same_bits(on_device[0].cpu().numpy(), prob) and same_bits(on_device[1].cpu().numpy(), defect)
    head = call(ref["energies"][:70])                                                    # an energy does not know its neighbours
    assert same_bits(head[0], prob[:70]) and same_bits(head[1], defect[:70])


# ---- 4. errors and the timer ---------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_write_nothing(gpu):
    import torch

    lib, dp = gpu.lib, C.POINTER(C.c_double)
    energies = np.linspace(3.0, 30.0, 5) ** 2 / 2.0 / MASS
    sentinel = -7.25
    prob, defect = np.full((5, 2, 2, 2), sentinel), np.full((5, 2), sentinel)
    ptr = lambda a: a.ctypes.data_as(dp)
    good = dict(num_pes=2, model=HN.SAC, mass=MASS, x_left=-40.0, x_right=40.0, n_steps=N_STEPS, n=5, energies=ptr(energies), flags=0, prob=ptr(prob),
                defect=ptr(defect))

    def status(**kw):
        a = {**good, **kw}
        return lib.gple_scatter(gpu.ctx, a["num_pes"], a["model"], a["mass"], a["x_left"], a["x_right"], a["n_steps"], a["n"], a["energies"], a["flags"], a["prob"],
                                a["defect"])

    bad_energy = energies.copy()
    bad_energy[3] = np.inf
    nan_energy = energies.copy()
    nan_energy[0] = np.nan
    where = torch.device("cuda", gpu.device)
    dev_bad = torch.from_numpy(bad_energy).to(where)
    dev_prob, dev_defect = torch.full((5, 2, 2, 2), sentinel, dtype=torch.float64, device=where), torch.full((5, 2), sentinel, dtype=torch.float64, device=where)
    torch.cuda.synchronize(where)
    cast = lambda t: C.cast(t.data_ptr(), dp)
    refused = [dict(num_pes=1), dict(num_pes=4), dict(model=HN.TSAC), dict(model=99), dict(model=_capi.PES_USER + 3), dict(n=0), dict(n=(1 << 20) + 1),
               dict(n_steps=1), dict(n_steps=0), dict(n_steps=(1 << 24) + 1), dict(mass=0.0), dict(mass=-1.0), dict(mass=np.nan), dict(mass=np.inf),
               dict(x_left=40.0), dict(x_left=50.0), dict(x_left=np.nan), dict(x_right=np.inf), dict(x_left=-np.inf), dict(energies=ptr(bad_energy)),
               dict(energies=ptr(nan_energy)), dict(energies=None), dict(prob=None),
               dict(n_steps=40),  # h = 2: c (E_max - eps_min) = (4 / 12) 4000 (0.225 + 0.02) >= 1/2
               dict(energies=cast(dev_bad), flags=_capi.IO_DEVICE, prob=cast(dev_prob), defect=cast(dev_defect))]
    for kw in refused:
        assert status(**kw) == BAD_ARG, kw
    gpu.synchronize()
    assert (prob == sentinel).all() and (defect == sentinel).all()
    assert (dev_prob.cpu().numpy() == sentinel).all() and (dev_defect.cpu().numpy() == sentinel).all()
    assert status() == 0 and not (prob == sentinel).any() and not (defect == sentinel).any()
    assert status(defect=None) == 0
    with pytest.raises(ValueError):
        gpu.scatter(2, HN.SAC, MASS, -40.0, 40.0, N_STEPS, np.zeros((2, 2)))


def test_timer_counts_calls(gpu):
    ref = reference("sac", 70)
    gpu.enable_timing(True)
    try:
        before = gpu.timing(_capi.TIMER_SCATTER)[2], gpu.timing(_capi.TIMER_HOP_SMOOTH)[2]
        gpu.scatter(2, HN.SAC, MASS, -40.0, 40.0, N_STEPS, ref["energies"])
        gpu.scatter(2, HN.SAC, MASS, -40.0, 40.0, N_STEPS, ref["energies"][:1], want_defect=False)
        last, _, count = gpu.timing(_capi.TIMER_SCATTER)
        assert count == before[0] + 2 and last > 0.0 and gpu.timing(_capi.TIMER_HOP_SMOOTH)[2] == before[1]
    finally:
        gpu.enable_timing(False)


# ---- 5. the driver ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_driver_against_the_stand_in(gpu, tmp_path):
    kw = dict(model=scattering.SAC, num_pes=2, momenta=np.linspace(4.0, 30.0, 16), surface0=0, x_left=-10.0, x_right=10.0, n_steps=1200, richardson=True)
    res = scattering.run(gpu, out_dir=str(tmp_path / "device"), **kw)
    ref = scattering.run(SN.NumpyScatterApi(), out_dir=str(tmp_path / "numpy"), **kw)
    wide = scattering.run(SN.NumpyScatterApi(dtype=np.longdouble), **kw)
    # the pattern of the parity test on the combination itself; its floor carries the weights |16 / 15| + |1 / 15| of the two solutions
    tol = 64.0 * float(np.nanmax(np.abs(ref["prob"] - wide["prob"]))) + (17.0 / 15.0) * 1e-13
    err = float(np.nanmax(np.abs(res["prob"] - ref["prob"])))
    print(f"scatter driver: err / tol {err / tol:.3g}, largest error estimate {np.nanmax(res['error']):.3g}")
    assert np.array_equal(np.isnan(res["prob"]), np.isnan(ref["prob"])) and err <= tol
    assert np.array_equal(res["head"], ref["head"]) and res["n_steps"] == 1200
    assert np.abs(res["error"] - ref["error"]).max() <= 2.0 * tol
    got, want = np.loadtxt(tmp_path / "device" / "smatrix.txt"), np.loadtxt(tmp_path / "numpy" / "smatrix.txt")
    assert got.shape == want.shape == (16, 6)
    assert np.allclose(got[:, :5], want[:, :5], rtol=2e-6, atol=2.0 * tol)  # "%g": six digits; the defect column is rounding alone
