"""GPU: the derivative members of a fit at and beyond n_total = 1024, member by member against the oracle.

real_fit_derivatives / complex_fit_derivatives (csrc/gple_capi.hip) change path at the padded size n_total (real: round_up(N, 256), complex:
2 round_up(N, 256)): up to 1024 the batched launches, above it a launch per product (gemv_partial + gemv_reduce, coldot, cderiv_diag on the two
Np x n_total x Np GEMMs E = A M_a, F = B M_b, and g x g grids of the auxiliary quadratic forms with g > 1).  tests/test_gpu_campaign.py stops at
n_total = 768 (real) / 1024 (complex); above that only the N = 4096 central difference of the summed objective looked, at 1e-4 and at the length
parameters.  Here: real N = 1000, 1024 (the batched path at its largest, with and without padded rows), 1025 (the first launch-per-product size, 255
padded rows), 1300; complex N = 513 (255 padded rows per half), 600.

Inputs and the complex references: oracle/gen_deriv_large.py (the literal complex oracle takes 16-25 s at these sizes, so its results are the fixtures
tests/golden/deriv_large_complex_*.npz, pinned to the oracle by tests/test_oracle_golden.py; the real oracle runs live, 1-4 s a case, once per session).

Tolerances: those of tests/test_gpu_campaign.py, unchanged but for one scale (next paragraph) — real: tol = max(1e-11, 100 cond(K) eps), 20 tol on derivative members, the purity
derivative priced against the purity / l it cancels; complex: tol = max(1e-10, 2000 cond(K) eps), 100 tol on the purity and the derivative members
(INVLBL_DERIV and the objective's gradient, which the campaign does not compare for complex fits, are derivative members).  cond(K) is that of the
reference's kernel matrix (1.5e5 .. 3.1e5 here: tol = 1.6e-9 .. 3.4e-9 real, 3.7e-8 complex); vectors are compared relative to their largest
component (component 0 of the real error derivative is analytically zero).  A 256-column chunk dropped or counted twice moves a member by 0.1 - 1
of its size.  The objective's reference is error + predictive error (and the same sum of the gradients): that is literally what the oracle's
loose_function returns (oracle/gple_oracle.cpp), without paying for a second fit.

One rule is wider than the campaign's, for a reason that lies in the reference: population_derivative.  Every entry of it is a constant times the
plain sum of a row of dv, and at these sizes those sums cancel to 1 / 1300 .. 1 / 3300 of their terms.  On the campaign's scale (20 tol of the
largest entry) library and oracle differ by 0.55, 0.09, 1.25 and 0.72 of the bound at N = 1000, 1024, 1025, 1300, all of it in the noise entry.
An evaluation in extended precision (K and the residuals of an iterative refinement in 80-bit long double, to 1e-15) settles whose it is: the
library's entries are within 3e-2 of that bound of it everywhere and its noise entry within 8e-5, the oracle's noise entry is 0.54, 0.09, 1.25
and 0.72 of the bound away.  The oracle follows the reference (kernel.cpp:358, 365-379): it forms the matrix dW = -2 sf^2 sn W W and then
dW y, so its noise row of dv carries the rounding of a squared inverse (0.26 of ITS bound, 20 tol of max |dv|, at N = 1025, where the
library's row is at 0.003), and the cancelling sum multiplies that by 1400; the library takes W (W y).  So the entry is priced against the terms
that cancel in it, as the campaign already prices the purity derivative; the ratio on the campaign's scale is printed beside it.  A dropped chunk
still misses the bound by four orders of magnitude and more (the last chunk left out of gemv_reduce_kernel, run once: 9e3 and 2e5 times the bound
at N = 1025 and 1300), and shows in dv itself (9e10 and 8e10 times its tolerance), which keeps the campaign's rule.

Every test prints its worst error / tolerance per quantity; DESIGN.md's parity section has the ratios measured on an MI355X."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from gaussian_process_liouville_equation_amd import _capi as c
from oracle import gen_deriv_large as gen
from tests import parity

pytestmark = pytest.mark.gpu
EPS = parity.EPS
REAL_SIZES = (1000, 1024, 1025, 1300)
COMPLEX_SIZES = gen.COMPLEX_SIZES
# the forced-tile children: the first launch-per-product size, n_total = 2048 (16 tile columns of 128: the XCD-aware tile order), complex E / F
CHILD_CASES = ((1025, False), (2000, False), (513, True))
REAL_DERIV = ("error_derivative", "population_derivative", "purity_derivative", "dv")
COMPLEX_DERIV = ("error_derivative", "purity_derivative", "dv")
INFO = " (campaign scale)"  # a ratio that is printed beside the judged one
_REAL_REFERENCE = {}


def members(api, N, cplx, validation=True, loose=True):
    """what a derivative fit of the case hands out (either backend): scalars, v = INVLBL, dv = INVLBL_DERIV, the predictive error and its
    derivative on the validation set, the objective and its gradient"""
    theta, X, y, Xv, yv = gen.deriv_large_inputs(N, cplx)
    fit = (api.complex_fit if cplx else api.real_fit)(theta, X, y, gen.FIT_FLAGS)
    out = dict(fit.scalars)
    out["v"] = fit.get(c.C_INVLBL if cplx else c.R_INVLBL).copy()
    out["dv"] = fit.get(c.C_INVLBL_DERIV if cplx else c.R_INVLBL_DERIV).copy()
    if not api.with_ctx:
        out["cond"] = np.linalg.cond(fit.get(c.C_KERNEL if cplx else c.R_KERNEL))
    if validation:
        pv = (api.complex_predict if cplx else api.real_predict)(fit, Xv, flags=c.CALC_DERIVATIVE, labels=yv, want=())
        out["v_error"], out["v_error_derivative"] = pv["error"], pv["error_derivative"]
    fit.release()
    if loose:
        out["loose"], out["loose_gradient"] = api.loose_function(theta, X, y.astype(complex), Xv, yv.astype(complex))
    return out


def pack(m, cplx):
    """the derivative members as one vector of doubles (the children's .npy); unpack() is its inverse"""
    return np.concatenate([np.ascontiguousarray(m[k]).view(np.float64).ravel() for k in (COMPLEX_DERIV if cplx else REAL_DERIV)])


def unpack(vec, N, cplx):
    out, at = {}, 0
    for k in (COMPLEX_DERIV if cplx else REAL_DERIV):
        if k == "dv":
            n = (16 if cplx else 4) * N
            out[k] = vec[at:at + n].view(np.complex128).reshape(8, N) if cplx else vec[at:at + n].reshape(4, N)
        else:
            n = 8 if cplx else 4
            out[k] = vec[at:at + n]
        at += n
    return out, at


def real_reference(oracle, N):
    if N not in _REAL_REFERENCE:
        ref = members(oracle, N, False, loose=False)
        assert ref["info"] == 0
        ref["loose"], ref["loose_gradient"] = ref["error"] + ref["v_error"], ref["error_derivative"] + ref["v_error_derivative"]
        _REAL_REFERENCE[N] = ref
    return _REAL_REFERENCE[N]


def complex_reference(N):
    ref = dict(np.load(gen.fixture_path(N)))
    ref["loose"], ref["loose_gradient"] = ref["error"] + ref["v_error"], ref["error_derivative"] + ref["v_error_derivative"]
    return ref


def _vec(got, ref, allowed, scale=None):
    """largest deviation over the allowed one, relative to the largest component of the reference"""
    scale = max(np.abs(ref).max(), 1e-300) if scale is None else scale
    return float(np.abs(np.asarray(got) - np.asarray(ref)).max() / (allowed * scale))


def real_ratios(got, ref, only=None):
    """tests/test_gpu_campaign.py, test_random_real_cases: error / tolerance per quantity"""
    tol = max(1e-11, 100.0 * float(ref["cond"]) * EPS)
    theta = gen.THETA_REAL
    r = {}
    for k in ("rescale_factor", "magnitude", "error", "population", "purity", "v_error", "loose"):
        r[k] = lambda k=k: abs(got[k] - ref[k]) / (tol * abs(ref[k]))
    for k in ("first_order_average", "v"):
        r[k] = lambda k=k: _vec(got[k], ref[k], tol)
    for k in ("error_derivative", "dv", "v_error_derivative", "loose_gradient"):
        r[k] = lambda k=k: _vec(got[k], ref[k], 20 * tol)
    # kernel.cpp:401-435: every entry is 2 pi sf^2 l0 l1 / s times the plain sum of a row of dv, and those sums cancel to 1 / 1300 .. 1 / 3300 of
    # their terms here (noise row at N = 1025: sum 0.112, sum of moduli 153) — priced against the terms that cancel, like the purity derivative
    # below; the module docstring has the measurement that made this necessary (it is the oracle's entry that is off, not the library's)
    factor = 2.0 * np.pi * theta[0] ** 2 * theta[1] * theta[2] / ref["rescale_factor"]
    cscale = max(np.abs(ref["population_derivative"]).max(), factor * np.abs(ref["dv"][1:]).sum(axis=1).max())
    r["population_derivative"] = lambda: _vec(got["population_derivative"], ref["population_derivative"], 20 * tol, cscale)
    r["population_derivative" + INFO] = lambda: _vec(got["population_derivative"], ref["population_derivative"], 20 * tol)  # printed, not judged
    # kernel.cpp:436-477: each entry is purity / l plus two sums of the opposite sign — priced against the purity / l it cancels
    pscale = max(np.abs(ref["purity_derivative"]).max(), abs(ref["purity"]) / min(theta[1], theta[2]))
    r["purity_derivative"] = lambda: _vec(got["purity_derivative"], ref["purity_derivative"], 20 * tol, pscale)
    return {k: f() for k, f in r.items() if only is None or k.replace(INFO, "") in only}, tol


def complex_ratios(got, ref, only=None):
    """tests/test_gpu_campaign.py, test_random_complex_cases"""
    tol = max(1e-10, 2000.0 * float(ref["cond"]) * EPS)
    r = {}
    for k in ("rescale_factor", "magnitude", "error", "v_error", "loose"):
        r[k] = lambda k=k: abs(got[k] - ref[k]) / (tol * abs(ref[k]))
    r["purity"] = lambda: abs(got["purity"] - ref["purity"]) / (100 * tol * abs(ref["purity"]))
    r["v"] = lambda: _vec(got["v"], ref["v"], tol)
    for k in ("error_derivative", "purity_derivative", "dv", "v_error_derivative", "loose_gradient"):
        r[k] = lambda k=k: _vec(got[k], ref[k], 100 * tol)
    return {k: f() for k, f in r.items() if only is None or k in only}, tol


def _judge(label, ratios, tol):
    print("%s: tol %.2e, worst error / tolerance: %s" % (label, tol, ", ".join("%s %.3g" % kv for kv in ratios.items())))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0 and not k.endswith(INFO)}  # (a NaN is bad)
    assert not bad, (label, bad)


@pytest.mark.parametrize("N", REAL_SIZES)
def test_real_derivative_fit_against_the_oracle(gpu, oracle, N):
    got, ref = members(gpu, N, False), real_reference(oracle, N)
    assert got["info"] == 0
    ratios, tol = real_ratios(got, ref)
    assert len(ratios) == 16
    _judge("real N = %d" % N, ratios, tol)


@pytest.mark.parametrize("N", COMPLEX_SIZES)
def test_complex_derivative_fit_against_the_oracle_fixture(gpu, N):
    got, ref = members(gpu, N, True), complex_reference(N)
    assert got["info"] == 0 and ref["dv"].shape == got["dv"].shape == (8, N)
    ratios, tol = complex_ratios(got, ref)
    assert len(ratios) == 12
    _judge("complex N = %d" % N, ratios, tol)


_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, %r)
import gaussian_process_liouville_equation_amd as pkg
from tests import test_gpu_deriv_large as t
api = pkg.open_api(0)
out = []
for N, cplx in t.CHILD_CASES:
    m = t.members(api, N, cplx, validation=False, loose=False)
    assert m["info"] == 0
    out.append(t.pack(m, cplx))
np.save(sys.argv[1], np.concatenate(out))
api.close()
"""


@pytest.mark.parametrize("name,env,tile", [("tile128", dict(GPLE_GEMM_128_MIN_TILES="1", GPLE_GEMM_SPLITK_MAX_TILES="0"), 128),
                                          ("splitk", dict(GPLE_GEMM_SPLITK_MAX_TILES="100000"), 32)])
def test_derivative_members_on_the_other_gemm_kernels(oracle, name, env, tile):
    """The dense derivative GEMMs of these sizes run on 64-tiles by default: 128-tiles take over at n_total >= 3072 and the split-k kernel stops at
    256 64-tiles.  The tile knobs are read once per process, so one child process per kernel runs real N = 1025, real N = 2000 (16 tile columns of
    128: the XCD-aware tile order) and complex N = 513 and writes the derivative members to an .npy; the parent compares them with the same
    references at the same tolerances (not with the default run's bits: the tile size changes the summation order).  GPLE_GEMM_LOG shows that the
    derivative products really ran on the kernel asked for.  A child that dies by a signal or runs into its time limit fails the test; nothing is
    tried again."""
    from tests.conftest import ROOT
    with tempfile.TemporaryDirectory() as d:
        f, log = os.path.join(d, "members.npy"), os.path.join(d, "gemm.log")
        res = subprocess.run([sys.executable, "-c", _CHILD % ROOT, f], env=dict(os.environ, GPLE_GEMM_LOG=log, **env), cwd=ROOT, capture_output=True,
                             text=True, timeout=240)  # three fits and the start of a process: seconds
        assert res.returncode == 0, (res.returncode, res.stdout[-500:], res.stderr[-2000:])
        vec = np.load(f)
        lines = [ln.split() for ln in open(log)]
    # stream tile M N K batch krange lower_only flops: the dense derivative products dK W (real) and E / F (complex)
    for shape in (["1280"] * 3, ["2048"] * 3, ["768", "1536", "768"]):
        tiles = [int(ln[1]) for ln in lines if ln[2:5] == shape and ln[6:8] == ["0", "0"]]
        assert tiles and set(tiles) == {tile}, (shape, tiles)
    at = 0
    for N, cplx in CHILD_CASES:
        got, used = unpack(vec[at:], N, cplx)
        at += used
        ref = complex_reference(N) if cplx else real_reference(oracle, N)
        ratios, tol = (complex_ratios if cplx else real_ratios)(got, ref, only=COMPLEX_DERIV if cplx else REAL_DERIV)
        assert len(ratios) == (3 if cplx else 5)
        _judge("%s, %s N = %d" % (name, "complex" if cplx else "real", N), ratios, tol)
    assert at == len(vec)
