#!/usr/bin/env python3
"""gen_deriv_large.py — the complex references of tests/test_gpu_deriv_large.py as fixtures; writes tests/golden/deriv_large_complex_<N>.npz.

TEST INFRASTRUCTURE ONLY.  Run in the development container:  python oracle/gen_deriv_large.py

Derivative fits beyond n_total = 1024 (the launch-per-product path of csrc/gple_capi.hip) are compared with the C++ oracle.  The real
cases call it live (a second or three each); the literal complex oracle is O(35 N^3) — 16 s at N = 513 and 25 s at N = 600 on 8 threads —
which is too long inside a GPU test, so its results are stored here: the fit's scalars, v = INVLBL, dv = INVLBL_DERIV (8 x N complex),
cond(K) of its kernel matrix (it only scales tolerances) and the predictive error with its derivative on the validation set.  The inputs
are not stored: deriv_large_inputs() regenerates them from the seed.  tests/test_oracle_golden.py regenerates N = 513 and pins the file to it.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

THETA_REAL = [1.0, 0.7086, 0.7056, 0.05]
THETA_COMPLEX = [1.0, 1.1, 0.8, 0.7, 0.9, 0.7, 0.8, 0.05]
M_VALIDATION = 700
FIT_FLAGS = 7  # CALC_ERROR | CALC_AVERAGE | CALC_DERIVATIVE
COMPLEX_SIZES = (513, 600)
SCALARS = ("rescale_factor", "magnitude", "error", "purity", "error_derivative", "purity_derivative")


def deriv_large_inputs(N, complex_case):
    """theta, X, y, Xv, yv: a Gaussian wave packet sampled at N points (seed 7000 + N) and the 700 wider-spread points of the same draw as
    the validation set, labelled with the exact packet (times 0.5 exp(i (x + 10) / 2) for the complex kernel, as tests/test_gpu_campaign.py)"""
    from tests import parity
    X, y, Xv = parity.synthetic_real(N, M_VALIDATION, 7000 + N)
    yv = np.exp(-0.5 * (((Xv[:, 0] + 10.0) / 0.7086) ** 2 + ((Xv[:, 1] - 14.112) / 0.7056) ** 2)) / (2 * np.pi * 0.7086 * 0.7056)
    if not complex_case:
        return THETA_REAL, X, y, Xv, yv
    ph = lambda Z: np.exp(0.5j * (Z[:, 0] + 10.0))
    return THETA_COMPLEX, X, 0.5 * y * ph(X), Xv, 0.5 * yv * ph(Xv)


def complex_reference(oracle, N):
    """what a fixture holds, from oracle.complex_fit and oracle.complex_predict on deriv_large_inputs(N, True)"""
    from gaussian_process_liouville_equation_amd import _capi as c
    theta, X, y, Xv, yv = deriv_large_inputs(N, True)
    fit = oracle.complex_fit(theta, X, y, FIT_FLAGS)
    sc = fit.scalars
    assert sc["info"] == 0
    out = {k: np.asarray(sc[k], dtype=np.float64) for k in SCALARS}
    out["v"] = fit.get(c.C_INVLBL).copy()
    out["dv"] = fit.get(c.C_INVLBL_DERIV).copy()
    out["cond"] = np.float64(np.linalg.cond(fit.get(c.C_KERNEL)))
    pv = oracle.complex_predict(fit, Xv, flags=c.CALC_DERIVATIVE, labels=yv, want=())
    out["v_error"] = np.float64(pv["error"])
    out["v_error_derivative"] = np.asarray(pv["error_derivative"], dtype=np.float64)
    fit.release()
    return out


def fixture_path(N):
    return os.path.join(ROOT, "tests", "golden", "deriv_large_complex_%d.npz" % N)


if __name__ == "__main__":
    from oracle import binding
    ora = binding.load()
    for size in COMPLEX_SIZES:
        if sys.argv[1:] and str(size) not in sys.argv[1:]:
            continue
        np.savez(fixture_path(size), **complex_reference(ora, size))
        print("wrote", fixture_path(size), os.path.getsize(fixture_path(size)), "bytes", flush=True)
