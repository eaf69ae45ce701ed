"""GPU (MI355X): the double k-steps of rownormp_kernel in the second half of every diagonal 256-block (csrc/gple_predict.hip: 32 k-rows per barrier,
the B slab of the second step folded into the zero half of the stage, only live fragments read) against the untouched rownorm2_kernel, which
walks the same block in sixteen single steps.  Per accumulator the MFMAs and the sums behind them are the same in the same order, so every
output must agree bit for bit — at the smallest shapes that reach each new path, as a full request (static grid) and as a default one (pruned,
work queue).  One shape also goes against the extended-precision evaluation of tests/predict_reference.py, so that the two kernels cannot be
wrong together."""
import ctypes

import numpy as np
import pytest

from gaussian_process_liouville_equation_amd import _capi as c
from tests import predict_reference as PR
from tests.test_gpu_configs import THETA_C, THETA_R, config_inputs

pytestmark = pytest.mark.gpu

R3 = "rownorm3_kernel"  # takes the full request of a one- or two-tile factor up to 512 row blocks, whatever the knob says


def kernel(pipe, blocking, queue):
    return f"rownorm{'p' if pipe else '2'}_kernel<{blocking},{'true' if queue else 'false'}>"


# N, M, complex, blocking, kernel of the full request (None: the knob's).  The streaming kernels need row blocks x N-tiles > 160.
CASES = [
    (768, 7000, False, "4,4", None),    # three N-tiles, the smallest 4 x 4 case: the unit crosses two tile boundaries, a double step's prefetch goes to the next tile's step 0
    (1024, 5300, False, "4,4", None),   # four tiles: all four column groups of the waves end a tile in a different live range
    (512, 10500, False, "2,8", R3),     # 2 x 8 blocking, two tiles (work-queue mode; the full request of so few row blocks belongs to rownorm3_kernel)
    (512, 66000, False, "2,8", None),   # 2 x 8 blocking on the static grid: more than 512 row blocks
    (1300, 6000, False, "4,4", None),   # padded n_total (1536)
    (700, 9000, True, "4,4", None),     # complex: typed rows, n_total = 2 x 768
]


def draw_points(X, M, seed):
    """half of the points near the data, half far from it (many of those are pruned by the default request)"""
    rng = np.random.default_rng(seed)
    N = len(X)
    near = X[rng.integers(0, N, M // 2)] + rng.normal(0, 0.3, (M // 2, 2))
    far = X[rng.integers(0, N, M - M // 2)] + rng.normal(0, 6.0, (M - M // 2, 2))
    return np.concatenate([near, far])[rng.permutation(M)]


@pytest.mark.parametrize("N,M,cplx,blocking,full_kernel", CASES)
def test_double_diagonal_steps_have_the_bits_of_the_single_ones(gpu, N, M, cplx, blocking, full_kernel):
    X, y, _, _ = config_inputs(N, 64, 5, cplx=cplx)
    pts = draw_points(X, M, N + M)
    fit = gpu.complex_fit(THETA_C, X, y, 0) if cplx else gpu.real_fit(THETA_R, X, y, 0)
    pred = gpu.complex_predict if cplx else gpu.real_predict
    knob = gpu.lib.gple_debug_predict_knobs
    knob.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    out, ran = {}, {}
    try:
        for v in (0, 1):
            assert knob(gpu.ctx, v, -1) == 0
            full = pred(fit, pts, flags=c.PREDICT_FULL)
            ran[v, 0] = gpu.last_contraction_kernel()
            pruned = pred(fit, pts)
            ran[v, 1] = gpu.last_contraction_kernel()
            out[v] = (full, pruned)
    finally:
        knob(gpu.ctx, 2, -1)
    for v in (0, 1):
        assert ran[v, 0] == (full_kernel or kernel(v, blocking, False)), ran
        assert ran[v, 1] == kernel(v, blocking, True), ran
    for leg in (0, 1):
        for k in ("prediction", "variance", "cutoff"):
            assert np.array_equal(out[0][leg][k], out[1][leg][k]), (leg, k, np.abs(out[0][leg][k] - out[1][leg][k]).max())
    var = out[1][0]["variance"]
    assert np.isfinite(var).all() and np.isfinite(out[1][1]["variance"]).all() and (var < 0.5 * var.max()).any()
    fit.release()


def test_double_diagonal_steps_against_the_extended_precision_reference(gpu):
    """N = 768 (three tiles, 4 x 4), the full request of rownormp_kernel: the first 256 rows of the 7000 — every workgroup runs the same code on
    its own rows — against the long-double evaluation of the same operation on the same fp64 operands, within the per-row bound that
    tests/predict_reference.py derives from the number formats (the one tests/test_gpu_predict_rows.py holds this N to)."""
    N, M, R = 768, 7000, 256
    X, y, _, _ = config_inputs(N, 64, 5)
    pts = np.ascontiguousarray(draw_points(X, M, N + M))
    fit = gpu.real_fit(THETA_R, X, y, 0)
    assert fit.scalars["info"] == 0
    T, n_split, n = fit.debug_factor()
    assert (n_split, n) == (768, N)
    p = gpu.real_predict(fit, pts, flags=c.PREDICT_FULL)
    assert gpu.last_contraction_kernel() == kernel(1, "4,4", False)
    ref = PR.real_reference(THETA_R, T, fit.get(c.R_INVLBL), X, pts[:R])
    rv = PR.ratio(p["variance"][:R], ref["var"], ref["var_bound"])
    rm = PR.ratio(p["prediction"][:R], ref["mean"], ref["mean_bound"])
    print(f"  N = {N}, rows 0 ... {R - 1} of {M}: max |error| / bound: variance {rv:.2e}, mean {rm:.2e}")
    assert np.all(np.isfinite(p["variance"])) and rv <= 1.0 and rm <= 1.0, (rv, rm)
    fit.release()
