"""GPU: user potentials (gple_pes_define, gple_pes_undefine, gple_pes_diabatic_n; csrc/gple_pes_n.h table_diabatic_n) through
every solver that accepts one, against the float64 restatement tests/pes_table_numpy.py installed into the existing restatements
(tests/dvr_numpy.py, tests/mqcl_numpy.py, oracle/evolve_oracle_n.py).  Every tolerance is the one the existing test of the same entry point
uses, plus the table's own where the potential enters; the ratios measured on the MI355X are in DESIGN.md §16."""
import ctypes as C
import math
import types

import numpy as np
import pytest

from gaussian_process_liouville_equation_amd import _capi, exact, exact_mqcl, kernels as K, steploop
from oracle import evolve_oracle_n as ON
from tests import dvr_numpy as DN
from tests import mqcl_numpy as MN
from tests import pes_table_numpy as PT
from tests import test_gpu_mqcl as TM
from tests import test_gpu_recon as TR
from tests import test_gpu_step_loop as TS

pytestmark = pytest.mark.gpu
EPS = PT.EPS
BAD_ARG = 1
USER = _capi.PES_USER
dptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))


@pytest.fixture
def define(gpu, monkeypatch):
    """define(table) -> model id on the session's context, with the restatements patched to see the table under that id; everything defined
    is undefined again when the test ends"""
    ids, tables = [], {}
    PT.install(monkeypatch, tables)

    def make(table):
        model = gpu.pes_define(table.num_pes, *table.args())
        ids.append(model)
        tables[model] = table
        return model

    yield make
    for model in ids:
        gpu.pes_undefine(model)


@pytest.fixture(scope="module")
def tables():
    """the smooth tables of the solver tests, built once: a dual avoided crossing that is not in the library and a three-level model"""
    return {2: PT.function_table(PT.other_dac, -14.0, 14.0, 0.125), 3: PT.function_table(PT.three_level, -14.0, 14.0, 0.125)}


# ---- 1. the interpolant -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_pes", [2, 3])
@pytest.mark.parametrize("n", [2, 3, 65])
def test_interpolant_against_restatement(gpu, define, num_pes, n):
    rng = np.random.default_rng(100 * num_pes + n)
    table = PT.random_table(num_pes, n, rng)
    model = define(table)
    nodes = table.nodes()
    lo, hi = nodes[0], nodes[-1]
    x = np.concatenate([nodes, 0.5 * (nodes[:-1] + nodes[1:]), rng.uniform(lo, hi, 256), lo - table.dx * np.array([1e-9, 0.3, 2.5]),
                        hi + table.dx * np.array([1e-9, 0.3, 2.5]), [hi]])
    V, F = gpu.pes_diabatic_n(num_pes, model, x)
    Vr, Fr = table.diabatic(x)
    tol = table.tolerance(x)
    rv, rf = np.max(np.abs(V - Vr) / tol), np.max(np.abs(F - Fr) / (tol / table.dx))
    print(f"interpolant num_pes {num_pes} n {n}: value err / tol {rv:.3g}, derivative err / tol {rf:.3g}")
    assert (np.abs(V - Vr) <= tol).all() and (np.abs(F - Fr) <= tol / table.dx).all()
    assert np.array_equal(V, np.swapaxes(V, 1, 2)) and np.array_equal(F, np.swapaxes(F, 1, 2))
    V2, F2 = gpu.pes_diabatic_n(num_pes, model, x)
    assert np.array_equal(V, V2) and np.array_equal(F, F2)


def test_nodes_of_a_dyadic_table_come_back_bit_for_bit(gpu, define):
    table = PT.random_table(3, 65, np.random.default_rng(9), x_first=-4.0, dx=0.125)
    model = define(table)
    V, F = gpu.pes_diabatic_n(3, model, table.nodes()[:-1])
    assert np.array_equal(V, table.V[:-1])
    # outside, the force is the end node's derivative exactly
    _, F = gpu.pes_diabatic_n(3, model, np.array([-9.0, 11.0]))
    assert np.array_equal(-F[0], table.dV[0]) and np.array_equal(-F[1], table.dV[-1])


@pytest.mark.parametrize("num_pes,model", [(2, 0), (2, 1), (2, 2), (3, 0), (3, 1), (3, 2), (3, 3)])
def test_diabatic_of_the_built_in_models(gpu, num_pes, model):
    """gple_pes_diabatic_n for the built-in ids against the oracle's potentials, at the tolerances of test_n_level_pes_against_oracle"""
    x = np.concatenate([np.linspace(-12, -0.01, 150), np.linspace(0.01, 12, 150), [0.37, -2.5]])
    V, F = gpu.pes_diabatic_n(num_pes, model, x)
    Vo, Fo = ON.diabatic(x, model, num_pes)
    assert np.abs(V - Vo).max() <= 1e-14 * max(np.abs(Vo).max(), 1e-3)
    assert np.abs(F - Fo).max() <= 1e-11 * np.abs(Fo).max()


# ---- 2. adiabatic quantities --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_pes", [2, 3])
def test_adiabatic_quantities_on_a_table(gpu, define, tables, num_pes):
    table = tables[num_pes]
    model = define(table)
    x = np.concatenate([np.linspace(-15.5, 15.5, 301), [0.37, -2.5, -14.0, 14.0]])  # inside, on the ends and in both continuations
    E, F, NAC = gpu.pes_adiabatic_n(num_pes, model, x)
    Eo, _, Fo, No = ON.adiabatic(x, model, num_pes)
    Vo, _ = table.diabatic(x)
    tol_e = num_pes * table.tolerance(x).max(axis=(1, 2)) + 8 * EPS * np.abs(Vo).max()  # Weyl: |dE| <= ||dV||_2 <= num_pes max|dV|
    re = np.max(np.abs(E - Eo) / tol_e[:, None])
    rf, rn = np.abs(F - Fo).max() / (1e-11 * np.abs(Fo).max()), np.abs(NAC - No).max() / (1e-9 * np.abs(No).max())
    print(f"adiabatic num_pes {num_pes}: E err / tol {re:.3g}, F {rf:.3g}, NAC {rn:.3g}")
    assert (np.abs(E - Eo) <= tol_e[:, None]).all()
    assert np.abs(F - Fo).max() <= 1e-11 * np.abs(Fo).max()
    assert np.abs(NAC - No).max() <= 1e-9 * np.abs(No).max()
    for a, b in zip((E, F, NAC), gpu.pes_adiabatic_n(num_pes, model, x)):
        assert np.array_equal(a, b)


# ---- 3. DVR -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_pes", [2, 3])
def test_dvr_hamiltonian_on_a_table(gpu, define, tables, num_pes):
    table = tables[num_pes]
    model = define(table)
    n, x_first, mass = 47, -7.5, 2000.0
    dx = 15.0 / (n - 1)
    x = x_first + dx * np.arange(n)
    for boundary in (DN.REFLECTIVE, DN.PERIODIC):
        H, E, B = gpu.dvr_hamiltonian(num_pes, model, boundary, x_first, dx, n, mass)
        ref = DN.hamiltonian(num_pes, model, boundary, x_first, dx, n, mass)
        assert np.array_equal(H, H.T)
        row = np.abs(ref).max(axis=1, keepdims=True)
        Vd, _ = table.diabatic(x)
        V, tolV = np.zeros_like(ref), np.zeros_like(ref)
        tv = table.tolerance(x)
        for m in range(num_pes):
            for mm in range(num_pes):
                V[m * n + np.arange(n), mm * n + np.arange(n)] = Vd[:, m, mm]
                tolV[m * n + np.arange(n), mm * n + np.arange(n)] = tv[:, m, mm]
        tol = 4 * EPS * row + 16 * EPS * np.abs(V) + tolV  # the existing test's, plus the potential's own
        print(f"dvr_hamiltonian num_pes {num_pes} boundary {boundary}: err / tol {np.max(np.abs(H - ref) / tol):.3g}")
        assert (np.abs(H - ref) <= tol).all()
        # energies: the bits of gple_pes_adiabatic_n (the contract of include/gple.h); basis: orthonormal, the restatement's up to the sign
        assert np.array_equal(E, gpu.pes_adiabatic_n(num_pes, model, x)[0])
        assert np.abs(np.einsum("aji,ajk->aik", B, B) - np.eye(num_pes)).max() <= 1e-14
        Co = ON.adiabatic(x, model, num_pes)[1]
        assert np.abs(B - Co).max() <= 1e-10  # with the sign: these tables couple every state everywhere, so the convention's component is far from 0
        for k in range(num_pes):
            last = np.array([v[np.nonzero(v)[0][-1]] for v in B[:, :, k]])
            assert (last > 0).all()
        H2, E2, B2 = gpu.dvr_hamiltonian(num_pes, model, boundary, x_first, dx, n, mass)
        assert np.array_equal(H, H2) and np.array_equal(E, E2) and np.array_equal(B, B2)


def test_dvr_propagation_on_a_dac_table_stays_within_duhamel_of_dac(gpu, define):
    """||psi_tab(t) - psi_DAC(t)|| <= t / hbar max_a ||dV(x_a)||_F ||psi0|| + 2 (the propagation tolerance of test_propagation_against_expm):
    Duhamel for two Hermitian generators that differ by the block-diagonal dV"""
    model = define(PT.dac_table(1 / 16))
    num_pes, n, boundary, mass = 2, 96, DN.PERIODIC, 2000.0
    x_first, dx = -10.0, 20.0 / (n - 1)
    x = x_first + dx * np.arange(n)
    dV = gpu.pes_diabatic_n(2, model, x)[0] - gpu.pes_diabatic_n(2, 1, x)[0]
    gap = np.sqrt((dV ** 2).sum(axis=(1, 2))).max()
    assert 0.0 < gap <= (1 / 16) ** 4 / 384 * PT.DAC_F4 * 2 * (1 + 1e-6)  # (Frobenius norm of the three distinct entries' interpolation errors)
    g = DN.gaussian(x, -2.0, 15.0, 0.7)
    times = np.array([0.0, 10.0, 333.3, 2500.0])
    B = gpu.dvr_hamiltonian(num_pes, 1, boundary, x_first, dx, n, mass, want_h=False)[2]
    psi0 = np.concatenate([B[:, j, 0] * g for j in range(num_pes)])  # one start for both runs: the lower adiabatic state of DAC
    nrm = np.linalg.norm(psi0)
    psi = {}
    for m in (model, 1):
        H = gpu.dvr_hamiltonian(num_pes, m, boundary, x_first, dx, n, mass, want_states=False)[0]
        lam, U = np.linalg.eigh(H)
        psi[m] = gpu.dvr_propagate(num_pes, n, U, lam, psi0, times)
    for k, t in enumerate(times):
        bound = t * gap * nrm + 2 * 1e-10 * nrm
        err = np.linalg.norm(psi[model][k] - psi[1][k])
        print(f"dvr_propagate t = {t}: distance / bound {err / bound:.3g}")
        assert err <= bound
    assert np.linalg.norm(psi[model][-1] - psi[1][-1]) > 0.0


# ---- 4. MQCLE -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_pes, n, steps", [(2, 64, 100), (3, 61, 50)])
def test_mqcl_on_a_table(gpu, define, tables, num_pes, n, steps):
    model = define(tables[num_pes])
    x, p, lx, lp = TM.grid(n)
    bases = MN.Bases(x, model, num_pes)
    rng = np.random.default_rng(40 + n)
    starts = {"gauss": TM.gaussian(num_pes, x, p), "random": MN.random_hermitian(num_pes, n, rng)}
    # every basis pair, with the restatement's basis vectors aligned to the device's signs (as tests/test_gpu_mqcl.py does)
    rho = starts["random"]
    for frm in range(3):
        src = gpu.mqcl_transform(num_pes, model, x, rho, MN.DIABATIC, frm)
        for to in range(3):
            dev = gpu.mqcl_transform(num_pes, model, x, src, frm, to)
            ref = MN.transform(rho, bases, MN.DIABATIC, to)
            for a in range(num_pes):
                for b in range(num_pes):
                    if a != b:
                        sgn = np.where(np.einsum("ij,ij->i", dev[a, b], np.conj(ref[a, b])).real < 0, -1.0, 1.0)
                        ref[a, b] *= sgn[:, None]
            assert TM.rel(dev, ref) <= 1e-13, (frm, to, TM.rel(dev, ref))
            assert np.array_equal(dev, gpu.mqcl_transform(num_pes, model, x, src, frm, to))
    for name, rho in starts.items():
        dev = gpu.mqcl_evolve(num_pes, model, x, p, rho, 2000.0, lx, lp, 0.25, steps)
        ref = MN.evolve(rho, bases, p, 2000.0, lx, lp, 0.25, steps)
        print(f"mqcl_evolve num_pes {num_pes} n {n} {name}: err / tol {TM.rel(dev, ref) / TM.EVOLVE_TOL:.3g}")
        assert TM.rel(dev, ref) <= TM.EVOLVE_TOL
        assert np.array_equal(dev, gpu.mqcl_evolve(num_pes, model, x, p, rho, 2000.0, lx, lp, 0.25, steps))
    dx, dp = x[1] - x[0], p[1] - p[0]
    rho = MN.transform(starts["gauss"], bases, MN.ADIABATIC, MN.DIABATIC)
    adia, av, pops = gpu.mqcl_observe(num_pes, model, x, p, rho, 2000.0, dx, dp)
    radia, rav, rpops = MN.observe(rho, bases, x, p, 2000.0, dx, dp)
    assert TM.rel(adia, radia) <= 1e-13
    assert np.abs(av - rav).max() <= 1e-12 * np.abs(rav).max()
    assert np.abs(pops - rpops).max() <= 1e-13 * np.abs(rpops).max()
    for a, b in zip((adia, av, pops), gpu.mqcl_observe(num_pes, model, x, p, rho, 2000.0, dx, dp)):
        assert np.array_equal(a, b)


# ---- 5. the tick --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_pes", [2, 3])
def test_tick_on_a_table(gpu, oracle, define, tables, num_pes):
    model = define(tables[num_pes])
    dens = TS._case_n(num_pes, 32, 300 + num_pes, x_centre=-0.8)
    fg, fo = TS._fits_n(gpu, dens, num_pes), TS._fits_n(oracle, dens, num_pes)
    order = K.element_order(num_pes)

    def distribution(pts, i, j):
        pred = oracle.complex_predict if i != j else oracle.real_predict
        return np.asarray(pred(fo[order.index((i, j))], pts, want=("cutoff",))["cutoff"], dtype=complex)

    out = gpu.evolve_n(num_pes, fg, model, TS.MASS, TS.DT, dens)
    ref = ON.evolve(dens, TS.MASS, TS.DT, distribution, model, num_pes)
    for e in order:
        scale = max(np.abs(ref[e][1]).max(), np.abs(dens[e][1]).max())
        print(f"tick num_pes {num_pes} element {e}: r err / tol {np.abs(out[e][0] - ref[e][0]).max() / (1e-12 * np.abs(ref[e][0]).max()):.3g}, "
              f"rho err / tol {np.abs(out[e][1] - ref[e][1]).max() / (1e-8 * scale):.3g}")
        assert np.abs(out[e][0] - ref[e][0]).max() <= 1e-12 * np.abs(ref[e][0]).max()
        assert np.abs(out[e][1] - ref[e][1]).max() <= 1e-8 * scale, e
    again = gpu.evolve_n(num_pes, fg, model, TS.MASS, TS.DT, dens)
    for e in order:
        assert np.array_equal(out[e][0], again[e][0]) and np.array_equal(out[e][1], again[e][1])
    if num_pes == 2:
        # steploop sends a user id through the N-level entry point at two levels: the same bits, and gple_evolve itself refuses the id
        fits = dict(zip(order, fg))
        all_kernels = lambda i, j=None: types.SimpleNamespace(_fit=fits[(i, i if j is None else j)], _api=gpu)
        all_kernels.num_pes = 2
        loop = steploop.evolve(dens, TS.MASS, TS.DT, all_kernels, model, gpu)
        new = steploop.new_point_predict(dens[(1, 0)][0], 1, 0, TS.MASS, TS.DT, all_kernels, model, gpu)
        for e in order:
            assert np.array_equal(loop[e][0], out[e][0]) and np.array_equal(loop[e][1], out[e][1])
        direct = gpu.evolve_n(2, fg, model, TS.MASS, TS.DT, {(1, 0): (dens[(1, 0)][0], np.zeros(len(dens[(1, 0)][0]), dtype=complex))}, new_points=True)
        assert np.array_equal(new, direct[(1, 0)][1])
        with pytest.raises(_capi.GpleError):
            gpu.evolve(fg, model, TS.MASS, TS.DT, dens)


# ---- 6. reconstruction --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_pes", [2, 3])
def test_survey_on_a_table(gpu, define, tables, num_pes):
    """the energy-weighted sums (slots 5 and 6) with the helper's energies, through the existing survey check (which prints err / tol per slot)"""
    model = define(tables[num_pes])
    x, p, dx, dp = TR.grid(33, 29)
    TR.check_survey(gpu, num_pes, model, TR.random_hermitian(num_pes, 33, 29, np.random.default_rng(33 + num_pes)), x, p, dx, dp)
    TR.check_survey(gpu, num_pes, model, TR.packets(num_pes, x, p), x, p, dx, dp)


def test_reconstruct_accepts_a_user_model(gpu, define):
    """the prediction does not depend on the potential: a DAC table gives the built-in model's bits there, and the same sums twice"""
    model = define(PT.dac_table(1 / 16))
    x, p, dx, dp = TR.grid(16, 20)
    rho = TR.packets(2, x, p)
    rng = np.random.default_rng(3)
    X, b = np.ascontiguousarray(np.stack([rng.uniform(-4, 0, 12), rng.uniform(14, 26, 12)], axis=1)), rng.normal(size=12) * 1e-2
    planes = [(TR.HYPER, X, b), None, None, (TR.HYPER, X, b)]
    cross = [(np.array([1e-3, 0.8, 1.0 / TR.SX, 0.05, 1.0 / TR.SP]), X, b), None, None, None]
    for fn, pl in ((gpu.grid_reconstruct, planes), (gpu.grid_reconstruct_cross, cross)):
        pred, sums = fn(2, model, rho, x, p, TR.MASS, dx, dp, pl)
        pred1, sums1 = fn(2, 1, rho, x, p, TR.MASS, dx, dp, pl)
        assert np.array_equal(pred, pred1) and np.isfinite(sums).all() and sums.shape == sums1.shape
        pred2, sums2 = fn(2, model, rho, x, p, TR.MASS, dx, dp, pl)
        assert np.array_equal(pred, pred2) and np.array_equal(sums, sums2)


# ---- 7. the registry ----------------------------------------------------------------------------------------------------------------------
def test_registry(gpu):
    import torch

    import gaussian_process_liouville_equation_amd as pkg

    lib, ctx = gpu.lib, gpu.ctx
    t2, t3 = PT.random_table(2, 9, np.random.default_rng(1)), PT.random_table(3, 5, np.random.default_rng(2))
    x = np.linspace(-3.0, 3.0, 41)
    ids = [gpu.pes_define(2, *t2.args()) for _ in range(15)] + [gpu.pes_define(3, *t3.args())]
    other = pkg.open_api(0)
    try:
        assert ids == list(range(USER, USER + 16))
        reference = gpu.pes_diabatic_n(2, ids[4], x)

        def define_status(num_pes, x_first, dx, V, dV, n=None):
            model = C.c_int(-7)
            V, dV = np.ascontiguousarray(V), np.ascontiguousarray(dV)
            st = lib.gple_pes_define(ctx, num_pes, x_first, dx, len(V) if n is None else n, dptr(V), dptr(dV), 0, C.byref(model))
            assert st != 0 and model.value == -7
            return st

        assert define_status(2, *t2.args()) == BAD_ARG  # the seventeenth
        gpu.pes_undefine(ids[4])
        with pytest.raises(_capi.GpleError):
            gpu.pes_diabatic_n(2, ids[4], x)  # undefined now
        with pytest.raises(_capi.GpleError):
            gpu.pes_undefine(ids[4])
        # device-pointer tables give the bits of host-pointer ones, and the freed slot is the one reused
        again = gpu.pes_define(2, t2.x_first, t2.dx, torch.from_numpy(t2.V).cuda(), torch.from_numpy(t2.dV).cuda())
        assert again == ids[4]
        for a, b in zip(reference, gpu.pes_diabatic_n(2, again, x)):
            assert np.array_equal(a, b)
        # refused, with the registry as it was
        out = np.zeros(8 * len(x) * 9)
        nan, skew = t2.V.copy(), t2.V.copy()
        nan[3, 1, 1], skew[2, 0, 1] = np.nan, np.nextafter(skew[2, 1, 0], 1.0)
        gpu.pes_undefine(ids[7])  # (room for one, so that a refusal below is the argument's and not the full registry's)
        for st in (define_status(2, t2.x_first, t2.dx, nan, t2.dV), define_status(2, t2.x_first, t2.dx, t2.V, nan),
                   define_status(2, t2.x_first, t2.dx, skew, t2.dV), define_status(2, t2.x_first, t2.dx, t2.V, skew),
                   define_status(2, t2.x_first, 0.0, t2.V, t2.dV), define_status(2, t2.x_first, -0.5, t2.V, t2.dV),
                   define_status(2, t2.x_first, np.inf, t2.V, t2.dV), define_status(2, np.nan, t2.dx, t2.V, t2.dV),
                   define_status(2, t2.x_first, t2.dx, t2.V, t2.dV, n=1), define_status(4, t2.x_first, t2.dx, t2.V, t2.dV),
                   define_status(2, t2.x_first, t2.dx, t2.V, t2.dV, n=(1 << 20) + 1)):
            assert st == BAD_ARG
        for num_pes, model, api in ((3, ids[0], gpu), (2, ids[15], gpu), (2, ids[0], other), (2, ids[7], gpu), (2, USER + 16, gpu), (2, 15, gpu), (2, -1, gpu)):
            assert api.lib.gple_pes_diabatic_n(api.ctx, num_pes, model, dptr(x), len(x), 0, dptr(out), dptr(out)) == BAD_ARG, (num_pes, model)
            assert api.lib.gple_pes_adiabatic_n(api.ctx, num_pes, model, dptr(x), len(x), 0, dptr(out)) == BAD_ARG
            assert api.lib.gple_dvr_hamiltonian(api.ctx, num_pes, model, 0, -1.0, 0.1, 8, 2000.0, 0, None, dptr(out), None) == BAD_ARG
            assert api.lib.gple_mqcl_transform(api.ctx, num_pes, model, dptr(x), 8, 0, 1, 0, dptr(out), dptr(out)) == BAD_ARG
            assert api.lib.gple_grid_survey(api.ctx, num_pes, model, dptr(out), dptr(x), 8, dptr(x), 8, 2000.0, 0.1, 0.1, 0, dptr(out)) == BAD_ARG
            assert api.lib.gple_mqcl_evolve(api.ctx, num_pes, model, dptr(x), dptr(x), 8, 2000.0, 2.0, 2.0, 0.1, 1, 0, dptr(out)) == BAD_ARG
            assert api.lib.gple_mqcl_observe(api.ctx, num_pes, model, dptr(x), dptr(x), 8, 2000.0, 0.1, 0.1, 0, dptr(out), None, dptr(out), dptr(out)) == BAD_ARG
            planes, cross = (_capi.ReconPlane * 9)(), (_capi.ReconCrossPlane * 9)()
            assert api.lib.gple_grid_reconstruct(api.ctx, num_pes, model, dptr(out), dptr(x), 8, dptr(x), 8, 2000.0, 0.1, 0.1, planes, None, 0, None, dptr(out)) == BAD_ARG
            assert api.lib.gple_grid_reconstruct_cross(api.ctx, num_pes, model, dptr(out), dptr(x), 8, dptr(x), 8, 2000.0, 0.1, 0.1, cross, None, 0, None, dptr(out)) == BAD_ARG
        # (the same calls with a defined id of the right num_pes are accepted: what was refused above was the id)
        planes, cross = (_capi.ReconPlane * 9)(), (_capi.ReconCrossPlane * 9)()
        assert lib.gple_mqcl_evolve(ctx, 2, ids[0], dptr(x), dptr(x), 8, 2000.0, 2.0, 2.0, 0.1, 1, 0, dptr(out)) == 0
        assert lib.gple_mqcl_observe(ctx, 2, ids[0], dptr(x), dptr(x), 8, 2000.0, 0.1, 0.1, 0, dptr(out), None, dptr(out), dptr(out)) == 0
        assert lib.gple_grid_reconstruct(ctx, 2, ids[0], dptr(out), dptr(x), 8, dptr(x), 8, 2000.0, 0.1, 0.1, planes, None, 0, None, dptr(out)) == 0
        assert lib.gple_grid_reconstruct_cross(ctx, 2, ids[0], dptr(out), dptr(x), 8, dptr(x), 8, 2000.0, 0.1, 0.1, cross, None, 0, None, dptr(out)) == 0
        assert lib.gple_pes_adiabatic(ctx, ids[0], dptr(x), len(x), 0, dptr(out)) == BAD_ARG  # the two-level legacy entries keep refusing
        with pytest.raises(_capi.GpleError):
            gpu.evolve([None, None, None], ids[0], 2000.0, 1.0, {e: (np.zeros((1, 2)), np.zeros(1, dtype=complex)) for e in K.element_order(2)})
        with pytest.raises(_capi.GpleError):
            gpu.evolve_n(2, [None, None, None], ids[15], 2000.0, 1.0, {(0, 0): (np.zeros((1, 2)), np.zeros(1, dtype=complex))})
        for a, b in zip(reference, gpu.pes_diabatic_n(2, again, x)):
            assert np.array_equal(a, b)
        assert gpu.pes_define(2, *t2.args()) == ids[7]  # exactly one slot was free: nothing above registered anything
        assert define_status(2, *t2.args()) == BAD_ARG
        # the other context has a registry of its own
        mine = other.pes_define(2, *t2.args())
        assert mine == USER
        for a, b in zip(reference, other.pes_diabatic_n(2, mine, x)):
            assert np.array_equal(a, b)
    finally:
        other.close()  # (frees what it still has defined)
        for model in range(USER, USER + 16):
            lib.gple_pes_undefine(ctx, model)


# ---- 8. the drivers -----------------------------------------------------------------------------------------------------------------------
def test_exact_run_on_a_user_model(gpu, define, tables, tmp_path):
    model = define(tables[2])
    res = exact.run(gpu, model=model, num_pes=2, boundary=exact.PERIODIC, ln_energy=-1.0, dx=0.25, max_outputs=4, out_dir=str(tmp_path), write_phase="text")
    s = res["setup"]
    _, E, B = gpu.dvr_hamiltonian(2, model, exact.PERIODIC, s["x"][0], s["dx"], s["n_grids"], s["mass"], want_h=False)
    ref = DN.run_loop(2, model, exact.PERIODIC, s, 4, (E, B))
    assert len(res["records"]) == len(ref) == 4
    for a, b in zip(res["records"], ref):
        assert a["t"] == b["t"]
        assert np.abs(a["populations"] - b["populations"]).max() <= 1e-9
        for k in ("E", "x", "p"):
            assert abs(a[k] - b[k]) <= 1e-9 * max(1.0, abs(b[k])), (k, a[k], b[k])
        assert (np.abs(a["phase_averages"] - b["phase_averages"]) <= 1e-9 * np.maximum(1.0, np.abs(b["phase_averages"]))).all()
    avg = np.loadtxt(tmp_path / "averages.txt")
    assert avg.shape[0] == 4 and np.array_equal(avg[:, 0], [float("%g" % r["t"]) for r in res["records"]])
    line = res["final_line"].split()
    assert len(line) == 3 and line[0] == "%g" % s["p0"]  # a user model: p0, the else branch (log(E) is DAC's alone)


def test_exact_mqcl_run_on_a_user_model(gpu, define, tables, tmp_path):
    model = define(tables[2])
    kw = dict(dx=0.125, dt=1.0, xmin=-10.0, xmax=10.0, x0=-3.0, output_time=20.0)
    res = exact_mqcl.run(gpu, model=model, num_pes=2, ln_energy=0.0, out_dir=str(tmp_path), write_phase="text", max_outputs=2, **kw)
    s = res["setup"]
    assert s["n_grids"] == 161
    recs, adia = TM.numpy_run(model, 2, s, 2)
    assert len(res["records"]) == 3
    for r, (t, av, pops) in zip(res["records"], recs):
        assert r["t"] == t
        assert np.abs(np.array([r["E"], r["x"], r["p"]]) - av).max() <= 1e-10 * np.abs(av).max()
        assert np.abs(r["populations"] - pops).max() <= 1e-10
    avg = np.loadtxt(tmp_path / "averages.txt")
    want = np.array([[float("%g" % v) for v in [r["t"], r["E"], r["x"], r["p"], *r["populations"]]] for r in res["records"]])
    assert np.array_equal(avg, want)
    blocks = [b for b in open(tmp_path / "phase.txt").read().split("\n\n") if b.strip()]
    last = np.array([[float(v) for v in line.split()] for line in blocks[2].strip("\n").split("\n")])
    z = (last[:, 0::2] + 1j * last[:, 1::2]).reshape(2, 2, 161, 161)
    assert np.abs(z - adia).max() <= 1e-5 * np.abs(adia).max()
    assert res["final_line"].split()[0] == "%g" % s["p0"]
    assert math.isfinite(float(res["final_line"].split()[1]))
