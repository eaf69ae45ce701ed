"""ctypes view of include/gple.h.

`Api` binds one shared library that exports the gple.h entry points under a given prefix.  The product binds
libgple_hip.so with prefix "gple_" (see __init__.py); the test-only CPU oracle exports the same interface under
"oracle_" (without contexts or device pointers) and is bound by oracle/binding.py with this same class, so the
parity tests drive both sides with identical code.
"""
import ctypes as C
import weakref

import numpy as np

GPLE_OK = 0
GPLE_ERR_TIMEOUT = 6  # a draining call noticed that the one-launch factorisation had given up: the fit is recovered, work enqueued before it is NaN (include/gple.h)
CALC_ERROR = 0x1
CALC_AVERAGE = 0x2
CALC_DERIVATIVE = 0x4
IO_DEVICE = 0x100
EVOLVE_NEW_POINTS = 0x400  # gple_evolve: new_point_predict instead of a tick
FORMAT_JOIN = 0x1000  # gple_format_g: no blank before the first number of a line
HOP_REVERSE = 0x2000  # gple_hop_evolve: a frustrated hop reverses the momentum
HOP_ACCUMULATE = 0x4000  # gple_hop_bin: add to acc instead of clearing it first
HOP_BIN_ALL = 0x8000  # gple_hop_bin: finished trajectories are binned too
TIMER_HOP_BIN = 13  # gple_timer: the bin kernel of one gple_hop_bin call
TIMER_HOP_GROUPS = 14  # gple_timer: the step kernel of one gple_hop_evolve_groups call
TIMER_HOP_MF = 15  # gple_timer: the step kernel of one gple_hop_evolve_mf or gple_hop_evolve_groups_mf call
TIMER_HOP_SQC = 16  # gple_timer: the step kernel of one gple_hop_evolve_sqc or gple_hop_evolve_groups_sqc call
TIMER_HOP_MASH = 17  # gple_timer: the step kernel of one gple_hop_evolve_mash or gple_hop_evolve_groups_mash call
TIMER_HOP_BIN_MF = 18  # gple_timer: the bin kernel of one gple_hop_bin_mf call
TIMER_HOP_OUTGOING = 19  # gple_timer: the bin kernel of one gple_hop_outgoing, gple_hop_outgoing_mf or gple_hop_outgoing_sqc call
TIMER_HOP_SMOOTH = 20  # gple_timer: the three kernels of one gple_hop_smooth or gple_hop_smooth_mf call
TIMER_SCATTER = 21  # gple_timer: the march kernel of one gple_scatter call
SCATTER_MAX_ENERGIES, SCATTER_MAX_STEPS = 1 << 20, 1 << 24  # the bounds of gple_scatter
# GPLE_HOP_AXIS_*: what gple_hop_outgoing bins by, and the names Api.hop_outgoing takes for them
HOP_AXIS_MOMENTUM, HOP_AXIS_ENERGY = range(2)
HOP_AXIS_NAMES = {"momentum": HOP_AXIS_MOMENTUM, "energy": HOP_AXIS_ENERGY}
HOP_MAX_GROUPS = 65536  # GPLE_HOP_MAX_GROUPS
# GPLE_HOP_WINDOW_*: the windows of the symmetrical quasi-classical trajectories, the names Api.hop_sample_sqc / hop_observe_sqc take for them, and
# the customary zero-point parameter gamma of each
HOP_WINDOW_SQUARE, HOP_WINDOW_TRIANGLE = range(2)
HOP_WINDOW_NAMES = {"square": HOP_WINDOW_SQUARE, "triangle": HOP_WINDOW_TRIANGLE}
HOP_WINDOW_GAMMA = {HOP_WINDOW_SQUARE: (3.0 ** 0.5 - 1.0) / 2.0, HOP_WINDOW_TRIANGLE: 1.0 / 3.0}
# GPLE_HOP_DC_*: the decoherence correction of gple_hop_evolve_dc / gple_hop_evolve_groups_dc (step 6a), and the names Api.hop_evolve takes for them
HOP_DC_NONE, HOP_DC_EDC, HOP_DC_COLLAPSE_HOP, HOP_DC_COLLAPSE_ATTEMPT = range(4)
HOP_DC_NAMES = {"none": HOP_DC_NONE, "edc": HOP_DC_EDC, "collapse_hop": HOP_DC_COLLAPSE_HOP, "collapse_attempt": HOP_DC_COLLAPSE_ATTEMPT}
PES_USER = 16  # GPLE_PES_USER: first id of a user potential (gple_pes_define)
PREDICT_FULL = 0x200  # contract every test row (default: far rows whose contraction cannot move the variance are skipped)

# gple_real_array / gple_complex_array
R_KERNEL, R_INVERSE, R_INVLBL, R_INVLBL_DERIV, R_LABEL, R_INVERSE_DIAG = range(6)
C_KERNEL, C_PSEUDO, C_UPPER_LEFT, C_LOWER_LEFT, C_INVLBL, C_INVLBL_DERIV, C_LABEL = range(7)

_dp = C.POINTER(C.c_double)


class RealFitScalars(C.Structure):
    _fields_ = [
        ("rescale_factor", C.c_double),
        ("magnitude", C.c_double),
        ("error", C.c_double),
        ("population", C.c_double),
        ("first_order_average", C.c_double * 2),
        ("purity", C.c_double),
        ("error_derivative", C.c_double * 4),
        ("population_derivative", C.c_double * 4),
        ("purity_derivative", C.c_double * 4),
        ("info", C.c_int),
    ]


class ComplexFitScalars(C.Structure):
    _fields_ = [
        ("rescale_factor", C.c_double),
        ("magnitude", C.c_double),
        ("error", C.c_double),
        ("purity", C.c_double),
        ("error_derivative", C.c_double * 8),
        ("purity_derivative", C.c_double * 8),
        ("info", C.c_int),
    ]


class Element(C.Structure):
    """gple_element: the fit of one density-matrix element (exactly one of the two set, or neither)"""
    _fields_ = [("real", C.c_void_p), ("cplx", C.c_void_p)]


class OptOptions(C.Structure):
    _fields_ = [("xtol_rel", C.c_double), ("ftol_rel", C.c_double), ("xtol_abs", C.c_double), ("ftol_abs", C.c_double),
                ("initial_step", C.c_double), ("max_eval", C.c_int)]


OBJECTIVE_FN = C.CFUNCTYPE(C.c_double, C.c_uint, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p)           # nlopt_func
CONSTRAINT_FN = C.CFUNCTYPE(None, C.c_uint, C.POINTER(C.c_double), C.c_uint, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p)  # nlopt_mfunc


def _opt_options(maxeval=0, initial_step=0.5):
    return OptOptions(1e-5, 1e-5, 1e-15, 1e-15, initial_step, int(maxeval or 0))


def _search(lib, name, head, x0, lb, ub, maxeval, options, is_log=()):
    """The part every gple_*minimize_* call shares: `head` (callbacks and their data, or handles, then the counts) is followed by the box,
    the options (None: the reference's tolerances with this maxeval), the start point / minimiser, the minimum and the evaluation count.
    `head` keeps the callback objects referenced until the call returns.  -> (x, f, n_eval)"""
    x, lbv, ubv = _f64(x0).copy(), _f64(lb), _f64(ub)
    f, ne = C.c_double(), C.c_int()
    opt = _opt_options(maxeval) if options is None else options
    st = getattr(lib, "gple_" + name)(*head, _ptr(lbv), _ptr(ubv), *is_log, C.byref(opt), _ptr(x), C.byref(f), C.byref(ne))
    if st != GPLE_OK:
        raise GpleError(f"gple_{name}: status {st}")
    return list(x), f.value, ne.value


def _value_callback(fun):
    return OBJECTIVE_FN(lambda nn, xp, gp, data: float(fun([xp[i] for i in range(nn)])))


def _handles(objectives):
    return (C.c_void_p * len(objectives))(*[o.handle.value for o in objectives])


def minimize_neldermead(lib, fun, x0, lb, ub, maxeval=0, options=None):
    """the library's own Nelder-Mead (gple_minimize_neldermead) on a Python objective fun(x list) -> float; (x, f, n_eval)"""
    return _search(lib, "minimize_neldermead", (_value_callback(fun), None, len(x0)), x0, lb, ub, maxeval, options)


def minimize_auglag_eq(lib, fun, constraint, m, x0, lb, ub, maxeval=0, options=None):
    """the library's augmented-Lagrangian search: fun(x, want_grad) -> (f, grad or None); constraint(x, want_grad) ->
    (h (m,), grad (m*n,) row-major or None); returns (x, f, n_eval)"""
    def f_cb(nn, xp, gp, data):
        v, g = fun([xp[i] for i in range(nn)], bool(gp))
        if gp:
            for i in range(nn):
                gp[i] = g[i]
        return float(v)

    def h_cb(mm, rp, nn, xp, gp, data):
        h, g = constraint([xp[i] for i in range(nn)], bool(gp))
        for i in range(mm):
            rp[i] = h[i]
        if gp:
            for i in range(mm * nn):
                gp[i] = g[i]

    return _search(lib, "minimize_auglag_eq", (OBJECTIVE_FN(f_cb), None, CONSTRAINT_FN(h_cb), None, m, len(x0)), x0, lb, ub, maxeval, options)


def objective_minimize_neldermead(lib, objectives, x0, lb, ub, maxeval=0, options=None):
    """gple_objective_minimize_neldermead over resident objectives (same data, different contexts): vertices evaluated concurrently"""
    return _search(lib, "objective_minimize_neldermead", (_handles(objectives), len(objectives), len(x0)), x0, lb, ub, maxeval, options)


def minimize_direct_l(lib, fun, x0, lb, ub, maxeval=0, options=None):
    """the library's DIRECT-L (gple_minimize_direct_l, the GN_DIRECT_L stand-in) on a Python objective fun(x list) -> float; (x, f, n_eval)"""
    return _search(lib, "minimize_direct_l", (_value_callback(fun), None, len(x0)), x0, lb, ub, maxeval, options)


def objective_minimize_direct_l(lib, objectives, x0, lb, ub, is_log=None, maxeval=0, options=None):
    """gple_objective_minimize_direct_l over resident objectives (same data, different contexts): the new rectangle centres of an iteration
    are evaluated concurrently; is_log flags the coordinates that are logarithms of their parameter (the global tier's reparametrisation)"""
    n = len(x0)
    flags = (C.c_ubyte * n)(*[1 if (is_log is not None and is_log[i]) else 0 for i in range(n)])
    return _search(lib, "objective_minimize_direct_l", (_handles(objectives), len(objectives), n), x0, lb, ub, maxeval, options, is_log=(flags,))


class Points(C.Structure):
    """gple_points: the selected phase-space points of one density-matrix element"""
    _fields_ = [("r", C.POINTER(C.c_double)), ("rho", C.POINTER(C.c_double)), ("n", C.c_size_t)]


class ReconPlane(C.Structure):
    """gple_recon_plane: kernel, training points and weights K^-1 y of one real plane (N = 0: predicted as exactly 0)"""
    _fields_ = [("x", C.c_double * 4), ("X", C.POINTER(C.c_double)), ("b", C.POINTER(C.c_double)), ("N", C.c_size_t)]


class ReconCrossPlane(C.Structure):
    """gple_recon_cross_plane: the same for the cross-term kernel x = (w_d, w_g, a, c, b)"""
    _fields_ = [("x", C.c_double * 5), ("X", C.POINTER(C.c_double)), ("b", C.POINTER(C.c_double)), ("N", C.c_size_t)]


class NlmlProblem(C.Structure):
    """gple_nlml_problem: one problem of gple_nlml_batch, x = (w_d, w_g, a_x, a_p, -) or (w_d, w_g, a, c, b)"""
    _fields_ = [("x", C.c_double * 5), ("X", C.POINTER(C.c_double)), ("y", C.POINTER(C.c_double)), ("N", C.c_size_t)]


class NlmlFitPlane(C.Structure):
    """gple_nlml_fit_plane: training set, start values and box of one plane of gple_nlml_fit_planes"""
    _fields_ = [("X", C.POINTER(C.c_double)), ("y", C.POINTER(C.c_double)), ("N", C.c_size_t), ("start", C.c_double * 5), ("lb", C.c_double * 5),
                ("ub", C.c_double * 5)]


NLML_BATCH_MAX_N = 256  # GPLE_NLML_BATCH_MAX_N


class PredictScalars(C.Structure):
    _fields_ = [("error", C.c_double), ("error_derivative", C.c_double * 8)]


def scalars_to_dict(s):
    out = {}
    for name, _ in s._fields_:
        v = getattr(s, name)
        out[name] = np.array(list(v)) if hasattr(v, "__len__") else v
    return out


class GpleError(RuntimeError):
    pass


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(_dp)


def _points(X):
    """(N,2) array of phase-space points -> contiguous interleaved [x0,p0,x1,p1,...] (stdafx.h:153)."""
    X = _f64(X)
    if X.ndim != 2 or X.shape[1] != 2:
        raise ValueError("phase-space points must have shape (N, 2)")
    return X


def _cplx(y):
    return np.ascontiguousarray(y, dtype=np.complex128)


def _on_device(a):
    return hasattr(a, "data_ptr")


def _io(*arrays):
    """numpy arrays -> (host pointers, 0); torch tensors on the GPU (contiguous) -> (device pointers, IO_DEVICE).  The one place that turns an
    array argument into a pointer for the entry points that take either side"""
    dev = [a is not None and _on_device(a) and a.is_cuda for a in arrays]
    if any(dev):
        if not all(d or a is None for a, d in zip(arrays, dev)):
            raise ValueError("either every array is a device tensor or none is")
        for a in arrays:
            if a is not None and not a.is_contiguous():
                raise ValueError("device tensors must be contiguous")
        return [None if a is None else C.cast(a.data_ptr(), _dp) for a in arrays], IO_DEVICE
    return [None if a is None else a.ctypes.data_as(_dp) for a in arrays], 0


def _dvr_shapes(num_pes, n_grids, H=None, W=None, basis=None, psi0=None):
    """ValueError unless every array given has the shape of its place in a DVR system of dim = num_pes * n_grids"""
    dim = num_pes * n_grids
    for a, shape in ((H, (dim, dim)), (W, (n_grids,)), (basis, (n_grids, num_pes, num_pes)), (psi0, (dim,))):
        if a is not None and a.shape != shape:
            raise ValueError("H (dim, dim), W (n_grids,), basis (n_grids, num_pes, num_pes) and psi0 (dim,) with dim = num_pes * n_grids")


def _device_planes(t, shape, source):
    """ValueError unless the tensor t is what `source`(device_out=True) returns: contiguous float64 planes of this shape on the GPU"""
    if tuple(t.shape) != shape or not t.is_cuda or str(t.dtype) != "torch.float64" or not t.is_contiguous():
        raise ValueError(f"a tensor must be the contiguous float64 {shape} planes of {source}(device_out=True) on the GPU")


def _axis(v):
    """grid values: a device tensor as it is, anything else as a float64 array"""
    return v if _on_device(v) else _f64(v)


def _rho(rho, num_pes, n=None):
    """a density in the phase.txt layout, complex128 (num_pes, num_pes, nx, np) — (num_pes, num_pes, n, n) when the square grid's n is given:
    a device tensor as it is, anything else as a contiguous array"""
    if not _on_device(rho):
        rho = np.ascontiguousarray(rho, dtype=np.complex128)
    shape = tuple(rho.shape)
    if len(shape) != 4 or shape[:2] != (num_pes, num_pes) or (n is not None and shape[2:] != (n, n)):
        raise ValueError(f"rho must have shape (num_pes, num_pes, {'nx, np' if n is None else 'n, n'})")
    if _on_device(rho) and str(rho.dtype) != "torch.complex128":
        raise ValueError("rho must be a complex128 tensor")
    return rho


def _like(ref, shape, dtype=np.float64):
    """an empty output on the side `ref` lives on"""
    if _on_device(ref):
        import torch
        return torch.empty(shape, dtype=getattr(torch, np.dtype(dtype).name), device=ref.device)
    return np.empty(shape, dtype=dtype)


# ---- the signatures of include/gple.h, written once ------------------------------------------------------------------------------------------
# name without prefix -> (result type, argument types).  CTX stands for the leading gple_ctx* and FL for the `unsigned flags` argument that the
# CPU oracle's mirror of the interface (prefix "oracle_", with_ctx=False) does not have; a flags argument the oracle keeps is a plain `u`.
# Handles are void*, so that a c_void_p, its integer value and None all pass.  tests/test_capi_symbols.py checks every row against the header.
CTX, FL = "ctx", "fl"


def _signatures():
    st, i, u, sz, d, vp, ull, ip = C.c_int, C.c_int, C.c_uint, C.c_size_t, C.c_double, C.c_void_p, C.c_ulonglong, C.POINTER(C.c_int)
    szp, el, pts, opt = C.POINTER(C.c_size_t), C.POINTER(Element), C.POINTER(Points), C.POINTER(OptOptions)
    llp = C.POINTER(C.c_longlong)
    predict = [CTX, vp, _dp, sz, u, _dp, _dp, _dp, _dp, C.POINTER(PredictScalars)]
    sharded = [CTX, vp, _dp, sz, u, i, i, vp, _dp, _dp, _dp]
    dealt = [CTX, vp, _dp, sz, u, i, i, ip, vp, _dp, _dp, _dp]
    search = [_dp, _dp, opt, _dp, _dp, ip]  # lb, ub, options, x, fmin, n_eval
    return {
        # context and tracing
        "ctx_create": (st, [i, vp, C.POINTER(vp)]),
        "ctx_destroy": (st, [CTX]),
        "ctx_synchronize": (st, [CTX]),
        "ctx_trim": (st, [CTX, szp]),
        "status_string": (C.c_char_p, [i]),
        "ctx_last_error": (C.c_char_p, [CTX]),
        "ctx_enable_timing": (st, [CTX, i]),
        "ctx_get_timing": (st, [CTX, i, _dp, _dp, C.POINTER(C.c_long)]),
        "ctx_get_prune_stats": (st, [CTX, C.POINTER(ull), C.POINTER(ull), i]),
        # kernels, fits and predicts
        "real_gram": (st, [CTX, _dp, _dp, sz, _dp, sz, i, FL, _dp, _dp]),
        "complex_gram": (st, [CTX, _dp, _dp, sz, _dp, sz, i, FL, _dp, _dp, _dp, _dp]),
        "cutoff_factor": (st, [CTX, _dp, i, _dp, sz, FL, _dp]),
        "real_fit_create": (st, [CTX, _dp, _dp, _dp, i, sz, u, C.POINTER(RealFitScalars), C.POINTER(vp)]),
        "real_fit_get_scalars": (st, [vp, C.POINTER(RealFitScalars)]),
        "real_fit_retain": (st, [vp]),
        "real_fit_release": (st, [vp]),
        "real_fit_size": (sz, [vp]),
        "real_fit_get": (st, [vp, i, FL, _dp]),
        "real_predict": (st, predict),
        "complex_fit_create": (st, [CTX, _dp, _dp, _dp, sz, u, C.POINTER(ComplexFitScalars), C.POINTER(vp)]),
        "complex_fit_get_scalars": (st, [vp, C.POINTER(ComplexFitScalars)]),
        "complex_fit_retain": (st, [vp]),
        "complex_fit_release": (st, [vp]),
        "complex_fit_size": (sz, [vp]),
        "complex_fit_get": (st, [vp, i, FL, _dp]),
        "complex_predict": (st, predict),
        "predict_batch": (st, [CTX, el, sz, _dp, ip, sz, _dp]),
        # the grid-sharded predicts
        "shard_bounds": (st, [sz, i, i, szp, szp, szp]),
        "set_allgather_function": (st, [vp]),
        "real_predict_sharded": (st, sharded),
        "complex_predict_sharded": (st, sharded),
        "real_predict_dealt": (st, dealt),
        "complex_predict_dealt": (st, dealt),
        "deal_share": (st, [sz, i, i, ip, szp, szp, szp]),
        # the objective and the searches
        "loose_function": (st, [CTX, _dp, sz, _dp, _dp, sz, _dp, _dp, sz, _dp, _dp]),
        "objective_create": (st, [CTX, _dp, _dp, sz, _dp, _dp, sz, C.POINTER(vp)]),
        "objective_eval": (st, [vp, _dp, sz, _dp, _dp]),
        "objective_eval_part": (st, [vp, _dp, sz, i, i, _dp, _dp]),
        "objective_release": (st, [vp]),
        "minimize_neldermead": (st, [OBJECTIVE_FN, vp, u] + search),
        "objective_minimize_neldermead": (st, [C.POINTER(vp), sz, sz] + search),
        "minimize_direct_l": (st, [OBJECTIVE_FN, vp, u] + search),
        "objective_minimize_direct_l": (st, [C.POINTER(vp), sz, sz, _dp, _dp, C.POINTER(C.c_ubyte)] + search[2:]),
        "minimize_auglag_eq": (st, [OBJECTIVE_FN, vp, CONSTRAINT_FN, vp, u, u] + search),
        # the step loop
        "pes_adiabatic": (st, [CTX, i, _dp, sz, u, _dp]),
        "evolve": (st, [CTX, el, i, d, d, pts, u]),
        "evolve_n": (st, [CTX, i, el, i, d, d, pts, u]),
        "pes_adiabatic_n": (st, [CTX, i, i, _dp, sz, u, _dp]),
        "pes_define": (st, [CTX, i, d, d, sz, _dp, _dp, u, ip]),
        "pes_undefine": (st, [CTX, i]),
        "pes_diabatic_n": (st, [CTX, i, i, _dp, sz, u, _dp, _dp]),
        "markov_chain": (st, [CTX, el, sz, d, ull, _dp, sz, _dp]),
        "markov_chain_trace": (st, [CTX, el, sz, d, ull, _dp, sz, _dp, _dp]),
        # the NLML GP of test/gpr.cpp
        "nlml": (st, [CTX, _dp, _dp, _dp, sz, _dp, _dp]),
        "nlml_predict": (st, [CTX, _dp, _dp, _dp, sz, _dp, sz, FL, _dp]),
        "nlml_cross": (st, [CTX, _dp, _dp, _dp, sz, _dp, _dp]),
        "nlml_cross_predict": (st, [CTX, _dp, _dp, _dp, sz, _dp, sz, FL, _dp]),
        # exact DVR and MQCLE dynamics
        "dvr_hamiltonian": (st, [CTX, i, i, i, d, d, sz, d, u, _dp, _dp, _dp]),
        "dvr_propagate": (st, [CTX, i, sz, _dp, _dp, _dp, _dp, sz, _dp, u, _dp]),
        "wigner": (st, [CTX, i, i, sz, d, d, _dp, sz, _dp, sz, _dp, d, u, _dp, _dp]),
        "dvr_absorber": (st, [CTX, d, d, sz, d, d, d, d, u, _dp]),
        "dvr_propagator": (st, [CTX, i, sz, _dp, _dp, d, sz, u, _dp]),
        "dvr_apply": (st, [CTX, i, sz, _dp, _dp, sz, _dp, u, _dp]),
        "dvr_flux": (st, [CTX, i, sz, _dp, _dp, d, sz, _dp, sz, u, _dp, _dp]),
        "dvr_flux_apply": (st, [CTX, i, sz, _dp, _dp, sz, u, _dp]),
        "dvr_spectrum": (st, [CTX, i, sz, _dp, _dp, d, i, _dp, sz, _dp, _dp, sz, u, _dp, _dp, _dp]),
        "mqcl_transform": (st, [CTX, i, i, _dp, sz, i, i, u, _dp, _dp]),
        "mqcl_evolve": (st, [CTX, i, i, _dp, _dp, sz, d, d, d, d, sz, u, _dp]),
        "mqcl_observe": (st, [CTX, i, i, _dp, _dp, sz, d, d, d, u, _dp, _dp, _dp, _dp]),
        "mqcl_absorb": (st, [CTX, i, i, _dp, sz, _dp, sz, u, _dp, _dp]),
        "mqcl_evolve_absorbing": (st, [CTX, i, i, _dp, _dp, sz, d, d, d, d, sz, sz, _dp, sz, u, _dp, _dp]),
        # fewest-switches surface hopping
        "hop_sample": (st, [CTX, i, i, sz, sz, ull, d, d, d, d, i, u, _dp, _dp, _dp, ip, ip]),
        "hop_evolve": (st, [CTX, i, i, sz, sz, ull, d, d, sz, sz, d, d, u, _dp, _dp, _dp, ip, ip]),
        "hop_observe": (st, [CTX, i, i, sz, d, u, _dp, _dp, _dp, ip, ip, _dp]),
        "hop_bin": (st, [CTX, i, i, sz, d, d, sz, d, d, sz, u, _dp, _dp, _dp, ip, ip, llp]),
        "hop_density": (st, [CTX, i, sz, sz, d, d, sz, u, llp, _dp]),
        "hop_sample_groups": (st, [CTX, i, i, sz, sz, sz, ull, _dp, i, u, _dp, _dp, _dp, ip, ip]),
        "hop_evolve_groups": (st, [CTX, i, i, sz, sz, sz, ull, d, _dp, sz, sz, d, d, u, _dp, _dp, _dp, ip, ip, ip]),
        "hop_observe_groups": (st, [CTX, i, i, sz, sz, d, u, _dp, _dp, _dp, ip, ip, _dp]),
        "hop_evolve_dc": (st, [CTX, i, i, sz, sz, ull, d, d, sz, sz, d, d, i, d, u, _dp, _dp, _dp, ip, ip]),
        "hop_evolve_groups_dc": (st, [CTX, i, i, sz, sz, sz, ull, d, _dp, sz, sz, d, d, i, d, u, _dp, _dp, _dp, ip, ip, ip]),
        # Ehrenfest (mean-field) trajectories
        "hop_evolve_mf": (st, [CTX, i, i, sz, d, d, sz, d, d, u, _dp, _dp, _dp, ip]),
        "hop_evolve_groups_mf": (st, [CTX, i, i, sz, sz, d, _dp, sz, d, d, u, _dp, _dp, _dp, ip]),
        "hop_observe_mf": (st, [CTX, i, i, sz, d, u, _dp, _dp, _dp, ip, _dp]),
        "hop_observe_groups_mf": (st, [CTX, i, i, sz, sz, d, u, _dp, _dp, _dp, ip, _dp]),
        "hop_bin_mf": (st, [CTX, i, i, sz, d, d, sz, d, d, sz, u, _dp, _dp, _dp, ip, llp]),
        "hop_density_mf": (st, [CTX, i, sz, sz, d, d, sz, u, llp, _dp]),
        # symmetrical quasi-classical trajectories
        "hop_sample_sqc": (st, [CTX, i, i, sz, sz, ull, d, d, d, d, i, i, d, u, _dp, _dp, _dp, ip, ip]),
        "hop_sample_groups_sqc": (st, [CTX, i, i, sz, sz, sz, ull, _dp, i, i, d, u, _dp, _dp, _dp, ip, ip]),
        "hop_evolve_sqc": (st, [CTX, i, i, sz, d, d, sz, d, d, d, u, _dp, _dp, _dp, ip]),
        "hop_evolve_groups_sqc": (st, [CTX, i, i, sz, sz, d, _dp, sz, d, d, d, u, _dp, _dp, _dp, ip]),
        "hop_observe_sqc": (st, [CTX, i, i, sz, d, i, d, u, _dp, _dp, _dp, ip, _dp]),
        "hop_observe_groups_sqc": (st, [CTX, i, i, sz, sz, d, i, d, u, _dp, _dp, _dp, ip, _dp]),
        # MASH trajectories
        "hop_sample_mash": (st, [CTX, i, i, sz, sz, ull, d, d, d, d, i, u, _dp, _dp, _dp, ip, ip]),
        "hop_sample_groups_mash": (st, [CTX, i, i, sz, sz, sz, ull, _dp, i, u, _dp, _dp, _dp, ip, ip]),
        "hop_evolve_mash": (st, [CTX, i, i, sz, d, d, sz, d, d, u, _dp, _dp, _dp, ip, ip]),
        "hop_evolve_groups_mash": (st, [CTX, i, i, sz, sz, d, _dp, sz, d, d, u, _dp, _dp, _dp, ip, ip, ip]),
        # what left the box, per channel
        "hop_outgoing": (st, [CTX, i, i, sz, d, i, d, d, sz, u, _dp, _dp, _dp, ip, ip, llp]),
        "hop_outgoing_mf": (st, [CTX, i, i, sz, d, i, d, d, sz, u, _dp, _dp, _dp, ip, llp]),
        "hop_outgoing_sqc": (st, [CTX, i, i, sz, d, i, d, i, d, d, sz, u, _dp, _dp, _dp, ip, llp]),
        # the smoothed density
        "hop_smooth": (st, [CTX, i, i, sz, d, d, sz, d, d, sz, d, d, sz, u, _dp, _dp, _dp, ip, ip, _dp, llp]),
        "hop_smooth_mf": (st, [CTX, i, i, sz, d, d, sz, d, d, sz, d, d, sz, u, _dp, _dp, _dp, ip, _dp, llp]),
        # exact branching probabilities per energy
        "scatter": (st, [CTX, i, i, d, d, d, sz, sz, _dp, u, _dp, _dp]),
        # many NLML problems in one launch; the search of several planes in lock-step on it
        "nlml_batch": (st, [CTX, C.POINTER(NlmlProblem), sz, i, u, _dp, _dp, C.POINTER(_dp), ip]),
        "nlml_fit_planes": (st, [CTX, C.POINTER(NlmlFitPlane), sz, i, opt, _dp, _dp, ip, C.POINTER(_dp)]),
        # reconstruction of a gridded density
        "nlml_weights": (st, [CTX, _dp, _dp, _dp, sz, u, _dp]),
        "grid_survey": (st, [CTX, i, i, _dp, _dp, sz, _dp, sz, d, d, d, u, _dp]),
        "grid_select": (st, [CTX, i, _dp, _dp, sz, _dp, sz, i, i, sz, ull, u, ip, _dp, _dp, szp]),
        "grid_reconstruct": (st, [CTX, i, i, _dp, _dp, sz, _dp, sz, d, d, d, C.POINTER(ReconPlane), _dp, u, _dp, _dp]),
        "nlml_cross_weights": (st, [CTX, _dp, _dp, _dp, sz, u, _dp]),
        "grid_reconstruct_cross": (st, [CTX, i, i, _dp, _dp, sz, _dp, sz, d, d, d, C.POINTER(ReconCrossPlane), _dp, u, _dp, _dp]),
        # "%g" text of device-resident doubles
        "format_g_bound": (sz, [sz, sz, sz]),
        "format_g": (st, [CTX, _dp, sz, sz, sz, u, vp, sz, szp]),
        # and the doubles of such text
        "parse_g": (st, [CTX, vp, sz, u, _dp, sz, szp, szp, szp]),
        # csrc/gple_debug.h: the debug entry points the binding itself calls
        "debug_last_contraction_kernel": (C.c_char_p, [CTX]),
        "debug_fit_factor": (st, [vp, vp, _dp, sz, ip, ip, ip]),
    }


SIGNATURES = _signatures()
# every symbol include/gple.h declares (checked by tests/test_capi_symbols.py)
GPLE_SYMBOLS = [name for name in SIGNATURES if not name.startswith("debug_")]


def declare(lib, prefix, with_ctx=True):
    """Give every table row whose symbol `lib` exports under `prefix` its argtypes and restype, with the markers resolved: the oracle's mirror
    (with_ctx=False) has neither contexts nor the FL flags.  Declarations belong to the loaded library and are made once, when it is loaded or
    bound: no call site assigns them again."""
    filled = {CTX: [C.c_void_p], FL: [C.c_uint]} if with_ctx else {CTX: [], FL: []}
    for name, (restype, args) in SIGNATURES.items():
        f = getattr(lib, prefix + name, None)
        if f is not None:
            f.restype, f.argtypes = restype, [t for a in args for t in filled.get(a, [a])]


class _Fit:
    """Owns one fit handle of either backend (RAII, like the reference's value-semantic kernel objects)."""

    def __init__(self, api, handle, kind, N, scalars=None):
        self.api, self.handle, self.kind, self.N = api, handle, kind, N
        self._scalars = scalars  # None: deferred create, fetched (with a stream sync) when a getter first needs them
        api._fits.add(self)

    @property
    def scalars(self):
        if self._scalars is None:
            sc = RealFitScalars() if self.kind == "real" else ComplexFitScalars()
            self.api._check(self.api._fn(f"{self.kind}_fit_get_scalars")(self.handle, C.byref(sc)))
            self._scalars = scalars_to_dict(sc)
        return self._scalars

    def release(self):
        if self.handle:
            self.api._fn(f"{self.kind}_fit_release")(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    def debug_factor(self):
        """gple_debug_fit_factor (csrc/gple_debug.h): (T, n_split, N) with T[n, k] the padded n_total x n_total inverse Cholesky factor as the
        predict kernels read it — the 64 x 64 blocks above the diagonal are unwritten memory (NaN under GPLE_POISON_T=1)"""
        which = (None, self.handle) if self.kind == "complex" else (self.handle, None)
        nt, ns, N = C.c_int(), C.c_int(), C.c_int()
        fn = self.api.lib.gple_debug_fit_factor
        self.api._check(fn(*which, None, 0, C.byref(nt), C.byref(ns), C.byref(N)))
        buf = np.empty(nt.value * nt.value)
        self.api._check(fn(*which, _ptr(buf), buf.size, C.byref(nt), C.byref(ns), C.byref(N)))
        return buf.reshape(nt.value, nt.value).T, ns.value, N.value  # (the buffer is column-major: T(n, k) at [n + k n_total])

    def get(self, which):
        N = self.N
        if self.kind == "real":
            shape = {R_KERNEL: (N, N), R_INVERSE: (N, N), R_INVLBL: (N,), R_INVLBL_DERIV: (4, N), R_LABEL: (N,),
                     R_INVERSE_DIAG: (N,)}[which]
            buf = np.empty(int(np.prod(shape)), dtype=np.float64)
            self.api._fit_get(self, which, buf)
            # N x N matrices arrive column-major: viewed as a C-ordered numpy array that is the transpose
            return buf.reshape(shape).T.copy() if which in (R_KERNEL, R_INVERSE) else buf.reshape(shape)
        shape, cplx = {C_KERNEL: ((N, N), False), C_PSEUDO: ((N, N), True), C_UPPER_LEFT: ((N, N), True),
                       C_LOWER_LEFT: ((N, N), True), C_INVLBL: ((N,), True), C_INVLBL_DERIV: ((8, N), True),
                       C_LABEL: ((N,), True)}[which]
        buf = np.empty(int(np.prod(shape)) * (2 if cplx else 1), dtype=np.float64)
        self.api._fit_get(self, which, buf)
        arr = buf.view(np.complex128) if cplx else buf
        arr = arr.reshape(shape)
        return arr.T.copy() if which in (C_KERNEL, C_PSEUDO, C_UPPER_LEFT, C_LOWER_LEFT) else arr


class _Objective:
    """Owns one gple_objective handle (training and extra set resident on the device)."""

    def __init__(self, api, X, y, Xe, ye):
        self.api, self.handle = api, C.c_void_p()
        api._check(api.lib.gple_objective_create(api.ctx, _ptr(X), _ptr(y.view(np.float64)), len(X), _ptr(Xe), _ptr(ye.view(np.float64)),
                                                 len(Xe), C.byref(self.handle)))
        api._fits.add(self)  # released with the context, like the fits

    def _eval(self, name, x, split, want_grad):
        x = _f64(x)
        val = C.c_double()
        grad = np.empty(len(x)) if want_grad else None
        self.api._check(self.api._fn(name)(self.handle, _ptr(x), len(x), *split, C.byref(val), _ptr(grad)))
        return val.value, grad

    def __call__(self, x, want_grad=True):
        return self._eval("objective_eval", x, (), want_grad)

    def part(self, x, part, nparts, want_grad=True):
        """gple_objective_eval_part: this rank's share of the value and gradient (sum over the parts = the whole; make_normal after the sum)"""
        return self._eval("objective_eval_part", x, (int(part), int(nparts)), want_grad)

    def release(self):
        if self.handle:
            self.api.lib.gple_objective_release(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class Api:
    def __init__(self, lib, prefix, with_ctx, device=0, stream=None):
        self.lib, self.prefix, self.with_ctx = lib, prefix, with_ctx
        self.ctx = None
        self.device = int(device)
        self._fits = weakref.WeakSet()  # a context must outlive its fit handles: close() releases them first
        declare(lib, prefix, with_ctx)
        if with_ctx:
            ctx = C.c_void_p()
            self._check(lib.gple_ctx_create(int(device), C.c_void_p(stream), C.byref(ctx)))
            self.ctx = ctx

    # ---- plumbing --------------------------------------------------------------------------------------------
    def _fn(self, name):
        return getattr(self.lib, self.prefix + name)

    def trim(self):
        """Free the pooled device buffers no live fit owns; returns the number of bytes released."""
        n = C.c_size_t(0)
        self._check(self.lib.gple_ctx_trim(self.ctx, C.byref(n)))
        return n.value

    def _check(self, status):
        if status != GPLE_OK:
            msg = f"status {status}"
            if self.with_ctx:
                msg = self.lib.gple_status_string(status).decode()
                if self.ctx:
                    msg += ": " + self.lib.gple_ctx_last_error(self.ctx).decode()
            raise GpleError(msg)

    def _c(self):
        return [self.ctx] if self.with_ctx else []

    def _fl(self, flags=0):
        return [flags] if self.with_ctx else []

    def close(self):
        for f in list(self._fits):
            f.release()
        if self.ctx:
            self.lib.gple_ctx_destroy(self.ctx)
            self.ctx = None

    def enable_timing(self, on=True):
        self._check(self.lib.gple_ctx_enable_timing(self.ctx, int(on)))

    def timing(self, which):
        """(last_ms, total_ms, count) of a gple_timer: 0 = fit, 1 = predict call, 2 = fused predict kernel, 3 = derivative GEMM, 4 = Wigner kernel, 5 = MQCLE
        steps, 6 = the device work of the reconstruction entry points, 7 = the kernels of format_g, 8 = the kernels of parse_g, 9 = the products of dvr_propagator, 10 = the products of dvr_flux,
        11 = the device work of dvr_spectrum, 12 = the step kernel of hop_evolve, 13 = the bin kernel of hop_bin,
        14 = the step kernel of hop_evolve_groups (12 and 14 also with a decoherence correction), 15 = the step kernel of hop_evolve_mf and
        hop_evolve_groups_mf, 16 = the step kernel of hop_evolve_sqc and hop_evolve_groups_sqc, 17 = the step kernel of hop_evolve_mash and
        hop_evolve_groups_mash, 18 = the bin kernel of hop_bin_mf, 19 = the bin kernel of hop_outgoing, hop_outgoing_mf and hop_outgoing_sqc,
        20 = the three kernels of hop_smooth and hop_smooth_mf, 21 = the march kernel of scatter."""
        last, total, count = C.c_double(), C.c_double(), C.c_long()
        self._check(self.lib.gple_ctx_get_timing(self.ctx, which, C.byref(last), C.byref(total), C.byref(count)))
        return last.value, total.value, count.value

    def last_contraction_kernel(self):
        """Name of the kernel this context's last predict ran its variance contraction on (csrc/gple_debug.h; the roofline label of bench.py)."""
        return (self.lib.gple_debug_last_contraction_kernel(self.ctx) or b"").decode()

    def prune_stats(self, reset=False):
        """(contracted, seen) test rows of the pruned predicts in units of 128 rows since creation / the last reset."""
        a, b = C.c_ulonglong(), C.c_ulonglong()
        self._check(self.lib.gple_ctx_get_prune_stats(self.ctx, C.byref(a), C.byref(b), int(bool(reset))))
        return a.value, b.value

    def synchronize(self):
        if self.ctx:
            self._check(self.lib.gple_ctx_synchronize(self.ctx))

    def _fit_get(self, fit, which, buf):
        self._check(self._fn(f"{fit.kind}_fit_get")(fit.handle, which, *self._fl(), _ptr(buf)))

    # ---- KernelBase ------------------------------------------------------------------------------------------
    def real_gram(self, theta, left, right, same_features=False, derivative=False):
        theta, left, right = _f64(theta), _points(left), _points(right)
        R, Cc = len(left), len(right)
        K = np.empty(R * Cc)
        dK = np.empty(4 * R * Cc) if derivative else None
        self._check(self._fn("real_gram")(*self._c(), _ptr(theta), _ptr(left), R, _ptr(right), Cc, int(same_features),
                                          *self._fl(), _ptr(K), _ptr(dK)))
        K = K.reshape(Cc, R).T  # column-major R x C
        if derivative:
            return K, dK.reshape(4, Cc, R).transpose(0, 2, 1)
        return K

    def complex_gram(self, theta, left, right, same_features=False, derivative=False):
        """ComplexKernelBase: (K, Kt) or (K, Kt, dK[8], dKt[8]), R x C arrays"""
        theta, left, right = _f64(theta), _points(left), _points(right)
        R, Cc = len(left), len(right)
        K, Kt = np.empty(R * Cc), np.empty(2 * R * Cc)
        dK = np.empty(8 * R * Cc) if derivative else None
        dKt = np.empty(16 * R * Cc) if derivative else None
        self._check(self._fn("complex_gram")(*self._c(), _ptr(theta), _ptr(left), R, _ptr(right), Cc, int(same_features),
                                             *self._fl(), _ptr(K), _ptr(Kt), _ptr(dK), _ptr(dKt)))
        K, Kt = K.reshape(Cc, R).T, Kt.view(np.complex128).reshape(Cc, R).T
        if derivative:
            return K, Kt, dK.reshape(8, Cc, R).transpose(0, 2, 1), dKt.view(np.complex128).reshape(8, Cc, R).transpose(0, 2, 1)
        return K, Kt

    def predict_batch(self, elements, points, element_of_request):
        """gple_predict_batch: elements = list of _Fit or None; points (n,2); element_of_request (n,) ints -> complex (n,)"""
        pts = _points(points)
        idx = np.ascontiguousarray(element_of_request, dtype=np.int32)
        out = np.empty(2 * len(pts))
        self._check(self.lib.gple_predict_batch(self.ctx, self._elements(elements), len(elements), _ptr(pts), idx.ctypes.data_as(C.POINTER(C.c_int)), len(pts), _ptr(out)))
        return out.view(np.complex128)

    def _elements(self, fits):
        arr = (Element * max(1, len(fits)))()
        for i, f in enumerate(fits):
            if f is not None:
                setattr(arr[i], "real" if f.kind == "real" else "cplx", f.handle.value)
        return arr

    def pes_adiabatic(self, model, x):
        """(M, 6): E0, E1, F00, F10, F11, NAC01 of Tully's model `model` (0 SAC, 1 DAC, 2 ECR) at positions x"""
        x = _f64(x)
        out = np.empty(6 * len(x))
        self._check(self.lib.gple_pes_adiabatic(self.ctx, int(model), _ptr(x), len(x), 0, _ptr(out)))
        return out.reshape(-1, 6)

    def evolve(self, fits, model, mass, dt, density, new_points=False):
        """one tick of evolve(): fits = [fit(0,0) | None, fit(1,0) | None, fit(1,1) | None]; density = {(i, j): (r (n,2), rho (n,))}
        -> the same structure one tick later.  new_points: new_point_predict (evolve.cpp:425-443) at the given points instead — they
        stay where they are and rho becomes what the back-propagation predicts there from the fits alone (0 where uncoupled)."""
        order = [(0, 0), (1, 0), (1, 1)]
        return self._tick("evolve", (), order, [density[e] for e in order], fits, model, mass, dt, new_points)

    def _tick(self, name, head, order, pairs, fits, model, mass, dt, new_points):
        """gple_evolve / gple_evolve_n on copies of the (r, rho) pairs of the elements in `order`"""
        rs = [np.ascontiguousarray(np.asarray(pair[0], dtype=np.float64).reshape(-1, 2)).copy() for pair in pairs]
        rhos = [np.ascontiguousarray(np.asarray(pair[1], dtype=np.complex128)).copy() for pair in pairs]
        pts = (Points * len(order))()
        for k in range(len(order)):
            pts[k].r, pts[k].rho, pts[k].n = _ptr(rs[k]), _ptr(rhos[k].view(np.float64)), len(rs[k])
        self._check(self._fn(name)(self.ctx, *head, self._elements(fits), int(model), float(mass), float(dt), pts, EVOLVE_NEW_POINTS if new_points else 0))
        return {e: (rs[k], rhos[k]) for k, e in enumerate(order)}

    def pes_adiabatic_n(self, num_pes, model, x):
        """N-level adiabatic quantities at positions x: (E (M, N), F (M, N, N) symmetric, NAC (M, N, N) antisymmetric, NAC[j, k] = F[j, k] / (E_j - E_k))"""
        x = _f64(x)
        ne = num_pes * (num_pes + 1) // 2
        w = num_pes + 2 * ne
        out = np.empty(w * len(x))
        self._check(self.lib.gple_pes_adiabatic_n(self.ctx, int(num_pes), int(model), _ptr(x), len(x), 0, _ptr(out)))
        out = out.reshape(-1, w)
        E, F, NAC = out[:, :num_pes].copy(), np.zeros((len(x), num_pes, num_pes)), np.zeros((len(x), num_pes, num_pes))
        e = 0
        for k in range(num_pes):
            for l in range(k + 1):
                F[:, k, l] = F[:, l, k] = out[:, num_pes + e]
                NAC[:, k, l], NAC[:, l, k] = out[:, num_pes + ne + e], -out[:, num_pes + ne + e]
                e += 1
        return E, F, NAC

    # ---- user potentials (gple_pes_define; pes.py tabulates a function) ------------------------------------------------------------------
    def pes_define(self, num_pes, x_first, dx, V, dV):
        """gple_pes_define: register the table V, dV (n, num_pes, num_pes) of the diabatic matrix and its x derivative at x_first + dx k (numpy
        arrays, or contiguous float64 device tensors) -> the model id (>= PES_USER) every N-level entry point of this context accepts"""
        V, dV = (a if _on_device(a) else _f64(a) for a in (V, dV))
        if tuple(V.shape) != tuple(dV.shape) or len(V.shape) != 3 or tuple(V.shape[1:]) != (num_pes, num_pes):
            raise ValueError("V and dV must have shape (n, num_pes, num_pes)")
        (pv, pd), flags = _io(V, dV)
        model = C.c_int(-1)
        self._check(self.lib.gple_pes_define(self.ctx, int(num_pes), float(x_first), float(dx), int(V.shape[0]), pv, pd, flags, C.byref(model)))
        return model.value

    def pes_undefine(self, model):
        """gple_pes_undefine: free a user model (its id may be handed out again)"""
        self._check(self.lib.gple_pes_undefine(self.ctx, int(model)))

    def pes_diabatic_n(self, num_pes, model, x):
        """gple_pes_diabatic_n: (V (M, N, N), F = -dV/dx (M, N, N)) of any model, built-in or user, at positions x"""
        x = _f64(x)
        V, F = np.empty((len(x), num_pes, num_pes)), np.empty((len(x), num_pes, num_pes))
        self._check(self.lib.gple_pes_diabatic_n(self.ctx, int(num_pes), int(model), _ptr(x), len(x), 0, _ptr(V), _ptr(F)))
        return V, F

    # ---- exact DVR dynamics (schrodinger_equation/ of the reference; gple_dvr_* / gple_wigner) ----------------------------------------------
    DVR_REFLECTIVE, DVR_PERIODIC = 0, 1

    def dvr_hamiltonian(self, num_pes, model, boundary, x_first, dx, n_grids, mass, want_h=True, want_states=True):
        """gple_dvr_hamiltonian: (H (dim, dim) or None, energies (n, num_pes) or None, basis (n, num_pes, num_pes) or None, columns = states)"""
        dim = num_pes * n_grids
        H = np.empty((dim, dim)) if want_h else None
        E = np.empty((n_grids, num_pes)) if want_states else None
        B = np.empty((n_grids, num_pes, num_pes)) if want_states else None
        self._check(self.lib.gple_dvr_hamiltonian(self.ctx, int(num_pes), int(model), int(boundary), float(x_first), float(dx), int(n_grids), float(mass), 0, _ptr(H), _ptr(E),
                                                  _ptr(B)))
        return H, E, B

    def dvr_propagate(self, num_pes, n_grids, eigvec, eigval, psi0, times, basis=None, from_psi0=True):
        """gple_dvr_propagate: psi(t) = C exp(-i E t) C^T psi0 at every time (from_psi0=False: psi0 already holds c0 = C^T psi0);
        eigvec[r, k] = component r of eigenvector k (numpy.linalg.eigh); basis (n, num_pes, num_pes): adiabatic output.  -> (T, dim) complex"""
        eigvec, eigval, times = _f64(eigvec), _f64(eigval), _f64(np.atleast_1d(times))
        psi0 = _cplx(psi0)
        dim = num_pes * n_grids
        if eigvec.shape != (dim, dim) or eigval.shape != (dim,) or psi0.shape != (dim,):
            raise ValueError("eigvec (dim, dim), eigval (dim,) and psi0 (dim,) with dim = num_pes * n_grids")
        basis = None if basis is None else _f64(basis)
        out = np.empty((len(times), dim), dtype=np.complex128)
        self._check(self.lib.gple_dvr_propagate(self.ctx, int(num_pes), int(n_grids), _ptr(eigvec), _ptr(eigval), _ptr(psi0.view(np.float64)), _ptr(times),
                                                len(times), _ptr(basis), 0x800 if from_psi0 else 0, _ptr(out.view(np.float64))))
        return out

    def wigner(self, num_pes, boundary, x_first, dx, p, psi, energies=None, mass=0.0, phase=True, averages=False, device_out=False):
        """gple_wigner on psi (T, num_pes * n) complex: (P (T, num_pes, num_pes, n, n_p) complex or None, averages (T, 3) = (E, x, p) or None).
        device_out: P stays on the device (a complex128 tensor on the context's device; the call has completed when it returns) — the inputs go
        up as tensors and only the averages come back"""
        p = _f64(p)
        psi = _cplx(np.atleast_2d(psi))
        T = psi.shape[0]
        n = psi.shape[1] // num_pes
        en = None if energies is None else _f64(energies)
        if device_out and phase:
            import torch
            where = torch.device("cuda", self.device)
            up = lambda a: None if a is None else torch.from_numpy(a).to(where)
            P = torch.empty((T, num_pes, num_pes, n, len(p)), dtype=torch.complex128, device=where)
            av = torch.empty((T, 3), dtype=torch.float64, device=where) if averages else None
            tp, tpsi, ten = up(p), up(psi.view(np.float64)), up(en)
            torch.cuda.synchronize(where)  # the uploads, before the context's stream reads them
            (pp, ppsi, pen, pP, pav), flags = _io(tp, tpsi, ten, torch.view_as_real(P), av)
            self._check(self.lib.gple_wigner(self.ctx, int(num_pes), int(boundary), n, float(x_first), float(dx), pp, len(p), ppsi, T, pen, float(mass), flags, pP, pav))
            self.synchronize()
            return P, None if av is None else av.cpu().numpy()
        P = np.empty((T, num_pes, num_pes, n, len(p)), dtype=np.complex128) if phase else None
        av = np.empty((T, 3)) if averages else None
        self._check(self.lib.gple_wigner(self.ctx, int(num_pes), int(boundary), n, float(x_first), float(dx), _ptr(p), len(p), _ptr(psi.view(np.float64)), T,
                                         _ptr(en), float(mass), 0, None if P is None else _ptr(P.view(np.float64)), _ptr(av)))
        return P, av

    # ---- the absorbing boundary: absorber, propagator of n_steps RK4 steps, its application (gple_dvr_absorber / _propagator / _apply) --------
    def dvr_absorber(self, x_first, dx, n_grids, mass, xmin, xmax, length):
        """gple_dvr_absorber: W (n_grids,) >= 0 of pes.cpp:64-93 on the grid x_first + dx a; exactly 0 for xmin <= x <= xmax"""
        W = np.empty(int(n_grids))
        self._check(self.lib.gple_dvr_absorber(self.ctx, float(x_first), float(dx), int(n_grids), float(mass), float(xmin), float(xmax), float(length), 0, _ptr(W)))
        return W

    def dvr_propagator(self, num_pes, n_grids, H, W, dt, n_steps, device_out=False):
        """gple_dvr_propagator: U = P4(-(W + i H) dt / hbar)^n_steps, what n_steps classical RK4 steps apply, as a complex128 (dim, dim) array;
        W (n_grids,) or None.  device_out: U stays on the device, a float64 tensor (2, dim, dim) = (Re, Im) on the context's device (the call has
        completed when it returns) that dvr_apply accepts as it is"""
        num_pes, n_grids = int(num_pes), int(n_grids)
        dim = num_pes * n_grids
        H = _f64(H)
        W = None if W is None else _f64(W)
        _dvr_shapes(num_pes, n_grids, H, W)
        if device_out:
            import torch
            where = torch.device("cuda", self.device)
            tH = torch.from_numpy(H).to(where)
            tW = None if W is None else torch.from_numpy(W).to(where)
            U = torch.empty((2, dim, dim), dtype=torch.float64, device=where)
            torch.cuda.synchronize(where)  # the uploads, before the context's stream reads them
            (pH, pW, pU), flags = _io(tH, tW, U)
            self._check(self.lib.gple_dvr_propagator(self.ctx, num_pes, n_grids, pH, pW, float(dt), int(n_steps), flags, pU))
            self.synchronize()
            return U
        planes = np.empty((2, dim, dim))
        self._check(self.lib.gple_dvr_propagator(self.ctx, num_pes, n_grids, _ptr(H), _ptr(W), float(dt), int(n_steps), 0, _ptr(planes)))
        return planes[0] + 1j * planes[1]

    def dvr_apply(self, num_pes, n_grids, U, psi0, T, basis=None):
        """gple_dvr_apply: psi[k] = U^(k + 1) psi0 for k < T -> (T, dim) complex, adiabatic with basis (n, num_pes, num_pes).  U: a complex
        (dim, dim) array, or the device tensor of dvr_propagator(device_out=True) (psi0 and basis go up, psi comes back)"""
        num_pes, n_grids, T = int(num_pes), int(n_grids), int(T)
        dim = num_pes * n_grids
        psi0 = _cplx(psi0)
        if _on_device(U):  # the tensor form is what dvr_propagator(device_out=True) returns, nothing else
            _device_planes(U, (2, dim, dim), "dvr_propagator")
        elif tuple(np.shape(U)) not in ((dim, dim), (2, dim, dim)):
            raise ValueError("U (dim, dim) complex or (2, dim, dim) planes with dim = num_pes * n_grids")
        _dvr_shapes(num_pes, n_grids, psi0=psi0)
        basis = None if basis is None else _f64(basis)
        out = np.empty((T, dim), dtype=np.complex128)
        if T == 0:
            return out
        if _on_device(U):
            import torch
            tv = torch.from_numpy(psi0.view(np.float64)).to(U.device)
            tb = None if basis is None else torch.from_numpy(basis).to(U.device)
            tout = torch.empty((T, 2 * dim), dtype=torch.float64, device=U.device)
            torch.cuda.synchronize(U.device)
            (pU, pv, pb, po), flags = _io(U, tv, tb, tout)
            self._check(self.lib.gple_dvr_apply(self.ctx, num_pes, n_grids, pU, pv, T, pb, flags, po))
            self.synchronize()
            return tout.cpu().numpy().view(np.complex128)
        planes = _f64(U) if np.ndim(U) == 3 else np.stack([np.real(U), np.imag(U)]).astype(np.float64)
        planes = np.ascontiguousarray(planes)
        self._check(self.lib.gple_dvr_apply(self.ctx, num_pes, n_grids, _ptr(planes), _ptr(psi0.view(np.float64)), T, _ptr(basis), 0,
                                            _ptr(out.view(np.float64))))
        return out

    # ---- what the absorber took: the quadratic forms per channel and their application (gple_dvr_flux / _flux_apply) ---------------------------
    def dvr_flux(self, num_pes, n_grids, H, W, dt, n_steps, basis, n_left, device_out=False, want_u=True):
        """gple_dvr_flux: (U, G).  G (2 num_pes, dim, dim) complex Hermitian: Re psi^H G[c] psi is what channel c = side num_pes + k (side 0: the
        grid points a < n_left; k: the adiabatic state, column k of basis (n, num_pes, num_pes)) absorbs over n_steps RK4 steps from the diabatic
        psi, unscaled; the channels add up to |psi|^2 - |U psi|^2.  A figure may be slightly negative.  U as dvr_propagator, or
        None without want_u.  device_out: both stay on the device as float64 tensors, U (2, dim, dim) and G (2 num_pes, 2, dim, dim) = (Re, Im)
        planes, which dvr_apply and dvr_flux_apply accept as they are"""
        num_pes, n_grids = int(num_pes), int(n_grids)
        dim = num_pes * n_grids
        H, basis = _f64(H), _f64(basis)
        W = None if W is None else _f64(W)
        _dvr_shapes(num_pes, n_grids, H, W, basis)
        if device_out:
            import torch
            where = torch.device("cuda", self.device)
            tH, tb = torch.from_numpy(H).to(where), torch.from_numpy(basis).to(where)
            tW = None if W is None else torch.from_numpy(W).to(where)
            U = torch.empty((2, dim, dim), dtype=torch.float64, device=where) if want_u else None
            G = torch.empty((2 * num_pes, 2, dim, dim), dtype=torch.float64, device=where)
            torch.cuda.synchronize(where)  # the uploads, before the context's stream reads them
            (pH, pW, pb, pU, pG), flags = _io(tH, tW, tb, U, G)
            self._check(self.lib.gple_dvr_flux(self.ctx, num_pes, n_grids, pH, pW, float(dt), int(n_steps), pb, int(n_left), flags, pU, pG))
            self.synchronize()
            return U, G
        planes = np.empty((2, dim, dim)) if want_u else None
        G = np.empty((2 * num_pes, 2, dim, dim))
        self._check(self.lib.gple_dvr_flux(self.ctx, num_pes, n_grids, _ptr(H), _ptr(W), float(dt), int(n_steps), _ptr(basis), int(n_left), 0, _ptr(planes), _ptr(G)))
        return (planes[0] + 1j * planes[1] if want_u else None), G[:, 0] + 1j * G[:, 1]

    def dvr_flux_apply(self, num_pes, n_grids, G, psi):
        """gple_dvr_flux_apply: Re psi_t^H G[c] psi_t for the diabatic states psi (T, dim) or (dim,) -> (T, 2, num_pes), [t, side, surface],
        unscaled (a population is this times dx).  G: the complex (2 num_pes, dim, dim) array of dvr_flux, or its device tensor"""
        num_pes, n_grids = int(num_pes), int(n_grids)
        dim = num_pes * n_grids
        psi = np.atleast_2d(_cplx(psi))
        T = psi.shape[0]
        if psi.shape != (T, dim) or not 1 <= T <= 4096:
            raise ValueError("psi (T, dim) with dim = num_pes * n_grids and 1 <= T <= 4096")
        out = np.empty((T, 2, num_pes))
        if _on_device(G):
            _device_planes(G, (2 * num_pes, 2, dim, dim), "dvr_flux")
            import torch
            tv = torch.from_numpy(psi.view(np.float64)).to(G.device)
            tout = torch.empty((T, 2 * num_pes), dtype=torch.float64, device=G.device)
            torch.cuda.synchronize(G.device)
            (pG, pv, po), flags = _io(G, tv, tout)
            self._check(self.lib.gple_dvr_flux_apply(self.ctx, num_pes, n_grids, pG, pv, T, flags, po))
            self.synchronize()
            return tout.cpu().numpy().reshape(T, 2, num_pes)
        if tuple(np.shape(G)) != (2 * num_pes, dim, dim):
            raise ValueError("G (2 num_pes, dim, dim) complex with dim = num_pes * n_grids")
        planes = np.ascontiguousarray(np.stack([np.real(G), np.imag(G)], axis=1).astype(np.float64))
        self._check(self.lib.gple_dvr_flux_apply(self.ctx, num_pes, n_grids, _ptr(planes), _ptr(psi.view(np.float64)), T, 0, _ptr(out)))
        return out

    # ---- the spectrum of one absorbing run (gple_dvr_spectrum) -----------------------------------------------------------------------------------
    def dvr_spectrum(self, num_pes, n_grids, H, W, dt, levels, basis, n_left, psi0, energies, want_psi=False, want_remaining=True):
        """gple_dvr_spectrum: (density, psi_e, remaining).  density (n_E, 2, num_pes), [energy, side, surface]: what each channel of dvr_flux
        absorbed per unit of energy at the total energies `energies` (H's own zero) over the first 2^levels RK4 steps from the diabatic psi0,
        unscaled (times dx dt / (2 pi hbar): a population per unit energy); a figure may be slightly negative.  psi_e (n_E, dim)
        complex, with want_psi: sum_{k < 2^levels} e^{i E dt k / hbar} P^k psi0; remaining: |P^(2^levels) psi0|^2.  What is not asked for is None"""
        num_pes, n_grids = int(num_pes), int(n_grids)
        dim = num_pes * n_grids
        H, basis, psi0, energies = _f64(H), _f64(basis), _cplx(psi0), np.atleast_1d(_f64(energies))
        W = None if W is None else _f64(W)
        _dvr_shapes(num_pes, n_grids, H, W, basis, psi0)
        n_E = energies.size
        if energies.ndim != 1 or not 1 <= n_E <= 4096:
            raise ValueError("energies (n_E,) with 1 <= n_E <= 4096")
        density = np.empty((n_E, 2, num_pes))
        psi_e = np.empty((n_E, dim), dtype=np.complex128) if want_psi else None
        remaining = np.empty(1) if want_remaining else None
        self._check(self.lib.gple_dvr_spectrum(self.ctx, num_pes, n_grids, _ptr(H), _ptr(W), float(dt), int(levels), _ptr(basis), int(n_left),
                                               _ptr(psi0.view(np.float64)), _ptr(energies), n_E, 0, _ptr(density),
                                               None if psi_e is None else _ptr(psi_e.view(np.float64)), _ptr(remaining)))
        return density, psi_e, (float(remaining[0]) if want_remaining else None)

    # ---- exact branching probabilities per energy (gple_scatter) ---------------------------------------------------------------------------------
    def scatter(self, num_pes, model, mass, x_left, x_right, n_steps, energies, want_defect=True):
        """gple_scatter: (prob, defect) of the coupled-channel Schrodinger equation on `model` at the total energies `energies` (the potential's
        own zero; a numpy array, or a contiguous float64 tensor on the GPU, which gives device tensors back), by the renormalised Numerov method on
        x_left + n h, n = 0 ... n_steps, the potential constant beyond both ends.  prob (n_E, num_pes, 2, num_pes),
        [energy, incoming surface, side (0 reflected, 1 transmitted), final surface]: exactly 0 for a closed final channel, NaN for a closed
        incoming one.  defect (n_E, num_pes), or None without want_defect: the probability sum of an incoming channel minus one"""
        num_pes = int(num_pes)
        if _on_device(energies):
            if str(energies.dtype) != "torch.float64" or energies.dim() != 1:
                raise ValueError("energies must be a float64 tensor (n_E,)")
            import torch
            torch.cuda.synchronize(energies.device)  # whatever produced the energies, before the context's stream reads them
        else:
            energies = np.atleast_1d(_f64(energies))
        n_E = int(energies.shape[0])
        if len(energies.shape) != 1 or not 1 <= n_E <= SCATTER_MAX_ENERGIES:
            raise ValueError(f"energies (n_E,) with 1 <= n_E <= {SCATTER_MAX_ENERGIES}")
        prob = _like(energies, (n_E, num_pes, 2, num_pes))
        defect = _like(energies, (n_E, num_pes)) if want_defect else None
        (pe, pp, pd), flags = _io(energies, prob, defect)
        self._check(self.lib.gple_scatter(self.ctx, num_pes, int(model), float(mass), float(x_left), float(x_right), int(n_steps), n_E, pe, flags, pp, pd))
        if flags:
            self.synchronize()
        return prob, defect

    # ---- text output (gple_format_g) ------------------------------------------------------------------------------------------------------------
    def format_g(self, values, per_line, lines_per_block=0, join=False):
        """gple_format_g: the "%g" text of `values` — a numpy array or a contiguous device tensor, float64 or complex128 (read as (re, im) pairs) —
        with a blank before every number (join: not before the first of a line), a newline after every per_line numbers and an empty line after
        every lines_per_block lines (0: never).  -> a bytes-like object of exactly the text's length"""
        if _on_device(values):
            import torch
            if not values.is_contiguous():
                raise ValueError("device tensors must be contiguous")
            if values.dtype == torch.complex128:
                values = torch.view_as_real(values)
            if values.dtype != torch.float64 or not values.is_cuda:
                raise ValueError("values must be a float64 or complex128 tensor on the GPU")
            count = values.numel()
        else:
            values = np.ascontiguousarray(values)
            values = values.astype(np.complex128, copy=False).view(np.float64) if np.iscomplexobj(values) else _f64(values)
            count = values.size
        per_line, lines_per_block = int(per_line), int(lines_per_block)
        if per_line <= 0 or count % per_line:
            raise ValueError("the number of values must be a multiple of per_line")
        bound = self.lib.gple_format_g_bound(count, per_line, lines_per_block)
        length = C.c_size_t(0)
        flags = FORMAT_JOIN if join else 0
        if _on_device(values):
            import torch
            text = torch.empty(max(1, bound), dtype=torch.uint8, device=values.device)
            torch.cuda.synchronize(values.device)  # whatever produced the values, before the context's stream reads them
            self._check(self.lib.gple_format_g(self.ctx, C.cast(values.data_ptr(), _dp), count, per_line, lines_per_block, flags | IO_DEVICE,
                                               C.c_void_p(text.data_ptr()), bound, C.byref(length)))
            return memoryview(text[:length.value].cpu().numpy())
        text = np.empty(max(1, bound), dtype=np.uint8)
        self._check(self.lib.gple_format_g(self.ctx, _ptr(values), count, per_line, lines_per_block, flags, C.c_void_p(text.ctypes.data), bound, C.byref(length)))
        return memoryview(text)[:length.value]

    # ---- text input (gple_parse_g) -------------------------------------------------------------------------------------------------------------
    def parse_g(self, text, device_out=False):
        """gple_parse_g: the doubles of blank-separated decimal text, converted on the device, each correctly rounded.  text: a bytes-like object, a
        numpy uint8 array or a contiguous uint8 tensor on the GPU (any byte offset).  -> (values, lines): a numpy float64 array — with device_out
        or a device text a float64 tensor on the GPU — and the number of lines that hold a number.  One call counts, a second one converts.  A
        malformed token raises ValueError with its byte offset and its bytes."""
        if not _on_device(text):
            text = np.ascontiguousarray(text, dtype=np.uint8).ravel() if isinstance(text, np.ndarray) else np.frombuffer(text, dtype=np.uint8)
            if device_out:
                import torch
                text = torch.from_numpy(text if text.flags.writeable else text.copy()).cuda()
        on_device = _on_device(text)
        if on_device:
            import torch
            if text.dtype != torch.uint8 or not text.is_cuda or text.dim() != 1 or not text.is_contiguous():
                raise ValueError("a device text must be a contiguous one-dimensional uint8 tensor on the GPU")
            length, address, flags = text.numel(), text.data_ptr(), IO_DEVICE
            torch.cuda.synchronize(text.device)  # whatever produced the text, before the context's stream reads it
        else:
            length, address, flags = text.size, text.ctypes.data, 0
        pointer = C.c_void_p(address if length else None)
        count, lines, bad = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        self._check(self.lib.gple_parse_g(self.ctx, pointer, length, flags, None, 0, C.byref(count), C.byref(lines), None))
        values = torch.empty(count.value, dtype=torch.float64, device=text.device) if on_device else np.empty(count.value)
        if count.value:
            out = C.cast(values.data_ptr(), _dp) if on_device else _ptr(values)
            status = self.lib.gple_parse_g(self.ctx, pointer, length, flags, out, count.value, C.byref(count), C.byref(lines), C.byref(bad))
            if status != GPLE_OK and bad.value != C.c_size_t(-1).value:
                piece = text[bad.value:bad.value + 65]
                raise ValueError(f"malformed number at byte {bad.value}: {bytes(piece.cpu().numpy() if on_device else piece).split()[0]!r}")
            self._check(status)
        return values, lines.value

    # ---- exact MQCLE dynamics (liouville_equation/ of the reference; gple_mqcl_*) -------------------------------------------------------------
    MQCL_DIABATIC, MQCL_ADIABATIC, MQCL_FORCE = 0, 1, 2

    def mqcl_transform(self, num_pes, model, x, rho, frm, to, out=None):
        """gple_mqcl_transform: basis_transform[frm][to] of rho (num_pes, num_pes, n, n) complex; numpy in -> new numpy array out, device tensors
        in -> written into `out` (a tensor like rho; rho itself when None)"""
        x = _axis(x)
        n = int(x.shape[0])
        rho = _rho(rho, num_pes, n)
        if out is None:
            out = rho if _on_device(rho) else np.empty_like(rho)
        (px, pi, po), flags = _io(x, rho, out)
        self._check(self.lib.gple_mqcl_transform(self.ctx, int(num_pes), int(model), px, n, int(frm), int(to), flags, pi, po))
        return out

    def mqcl_evolve(self, num_pes, model, x, p, rho, mass, length_x, length_p, dt, n_steps):
        """gple_mqcl_evolve: n_steps Trotter steps on the diabatic rho (num_pes, num_pes, n, n) complex.  numpy: returns the evolved copy;
        device tensors: evolves rho in place (asynchronously on the context's stream) and returns it"""
        x, p = _axis(x), _axis(p)
        n = int(x.shape[0])
        rho = _rho(rho, num_pes, n)
        if not _on_device(rho):
            rho = rho.copy()
        (px, pp, pr), flags = _io(x, p, rho)
        self._check(self.lib.gple_mqcl_evolve(self.ctx, int(num_pes), int(model), px, pp, n, float(mass), float(length_x), float(length_p), float(dt), int(n_steps),
                                              flags, pr))
        return rho

    def mqcl_observe(self, num_pes, model, x, p, rho_dia, mass, dx, dp, adiabatic=True):
        """gple_mqcl_observe: (rho_adia (num_pes, num_pes, n, n) or None, averages (E, x, p), populations (num_pes,)); with device tensors the
        three outputs are device tensors"""
        x, p = _axis(x), _axis(p)
        n = int(x.shape[0])
        rho_dia = _rho(rho_dia, num_pes, n)
        adia = _like(rho_dia, rho_dia.shape, np.complex128) if adiabatic else None
        av, pops = _like(rho_dia, 3), _like(rho_dia, num_pes)
        (px, pp, pr, pa, pav, ppo), flags = _io(x, p, rho_dia, adia, av, pops)
        self._check(self.lib.gple_mqcl_observe(self.ctx, int(num_pes), int(model), px, pp, n, float(mass), float(dx), float(dp), flags, pr, pa, pav, ppo))
        return adia, av, pops

    def _mqcl_mask(self, num_pes, n, rho, g, absorbed_p):
        """the state, the half-mask g (n,) and the accumulator (2, num_pes, n) of a masking call, on one side: numpy -> copies of the state and
        the accumulator (zeros when None), device tensors as they are (the accumulator a new zero tensor when None)"""
        rho = _rho(rho, num_pes, n)
        g = _axis(g)
        if tuple(g.shape) != (n,):
            raise ValueError("g has one value per grid point")
        if absorbed_p is None:
            absorbed_p = _like(rho, (2, num_pes, n))
            absorbed_p[...] = 0.0
        elif not _on_device(absorbed_p):
            absorbed_p = np.array(absorbed_p, dtype=np.float64, order="C")
        if tuple(absorbed_p.shape) != (2, num_pes, n) or (_on_device(absorbed_p) and str(absorbed_p.dtype) != "torch.float64"):
            raise ValueError("absorbed_p is float64 of shape (2, num_pes, n)")
        if not _on_device(rho):
            rho = rho.copy()
        return rho, g, absorbed_p

    def mqcl_absorb(self, num_pes, model, x, rho, g, n_left, absorbed_p=None):
        """gple_mqcl_absorb: rho(x_i, .) <- (1 - g_i) rho(x_i, .) on the diabatic rho (num_pes, num_pes, n, n) complex, and g_i times the adiabatic
        diagonal added to absorbed_p (2, num_pes, n) [side][surface][j], side 0 the rows i < n_left; absorbed_p None starts from zeros.  numpy:
        returns the masked copy and the new accumulator; device tensors: both in place (asynchronously) and returned"""
        x = _axis(x)
        n = int(x.shape[0])
        rho, g, absorbed_p = self._mqcl_mask(num_pes, n, rho, g, absorbed_p)
        (px, pg, pr, pa), flags = _io(x, g, rho, absorbed_p)
        self._check(self.lib.gple_mqcl_absorb(self.ctx, int(num_pes), int(model), px, n, pg, int(n_left), flags, pr, pa))
        return rho, absorbed_p

    def mqcl_evolve_absorbing(self, num_pes, model, x, p, rho, mass, length_x, length_p, dt, n_steps, mask_every, g, n_left, absorbed_p=None):
        """gple_mqcl_evolve_absorbing: n_steps / mask_every blocks of mqcl_absorb(g), mask_every steps of mqcl_evolve, mqcl_absorb(g), enqueued in
        one call; the bits of those separate calls.  Arrays and results as mqcl_absorb"""
        x, p = _axis(x), _axis(p)
        n = int(x.shape[0])
        rho, g, absorbed_p = self._mqcl_mask(num_pes, n, rho, g, absorbed_p)
        (px, pp, pg, pr, pa), flags = _io(x, p, g, rho, absorbed_p)
        self._check(self.lib.gple_mqcl_evolve_absorbing(self.ctx, int(num_pes), int(model), px, pp, n, float(mass), float(length_x), float(length_p), float(dt),
                                                        int(n_steps), int(mask_every), pg, int(n_left), flags, pr, pa))
        return rho, absorbed_p

    # ---- fewest-switches surface hopping (gple_hop_*; DESIGN.md §17, driven by hopping.py) -----------------------------------------------------
    # An ensemble is the tuple (x (n,), p (n,) float64, b (n, num_pes) complex128 diabatic amplitudes, surface (n,), status (n,) int32): numpy
    # arrays, or contiguous tensors on the context's device
    def _hop_state(self, num_pes, state):
        x, p, b, surface, status = state
        if _on_device(x):
            kinds = ("torch.float64", "torch.float64", "torch.complex128", "torch.int32", "torch.int32")
            if not all(_on_device(a) and a.is_cuda and a.is_contiguous() and str(a.dtype) == kind for a, kind in zip(state, kinds)):
                raise ValueError("a device ensemble is contiguous float64 x, p, complex128 b and int32 surface, status tensors on the GPU")
        else:
            x, p, b = _f64(x), _f64(p), _cplx(b)
            surface, status = (np.ascontiguousarray(a, dtype=np.int32) for a in (surface, status))
        n = int(x.shape[0])
        if n < 1 or any(tuple(a.shape) != (n,) for a in (x, p, surface, status)) or tuple(b.shape) != (n, num_pes):
            raise ValueError("an ensemble is x, p, surface, status of shape (n,) and b of shape (n, num_pes), n >= 1")
        return (x, p, b, surface, status), n

    @staticmethod
    def _hop_pointers(state):
        (px, pp, pb), flags = _io(*state[:3])
        ip = C.POINTER(C.c_int)
        return [px, pp, pb] + [C.cast(a.data_ptr(), ip) if flags else a.ctypes.data_as(ip) for a in state[3:]], flags

    # The shared bodies.  Every gple_hop_* function is (ctx, num_pes, <head>, flags, <the ensemble's pointers>, <tail>); `name` is the C name
    # without its gple_, pointers_of is _hop_pointers, or _hop_mf_pointers for the calls that are never given the surface
    def _hop_call(self, name, num_pes, head, state, pointers_of, flags=0, tail=()):
        pointers, io = pointers_of(state)
        self._check(getattr(self.lib, "gple_" + name)(self.ctx, int(num_pes), *head, flags | io, *pointers, *tail))

    def _hop_own(self, num_pes, state):
        """_hop_state for a step that writes all five arrays: a numpy ensemble is copied, a device one is evolved in place"""
        state, n = self._hop_state(int(num_pes), state)
        return (state if _on_device(state[0]) else tuple(a.copy() for a in state)), n

    def _hop_empty(self, num_pes, n, device_out):
        if device_out:
            import torch
            where = torch.device("cuda", self.device)
            return (torch.empty(n, dtype=torch.float64, device=where), torch.empty(n, dtype=torch.float64, device=where),
                    torch.empty((n, num_pes), dtype=torch.complex128, device=where), torch.empty(n, dtype=torch.int32, device=where),
                    torch.empty(n, dtype=torch.int32, device=where))
        return (np.empty(n), np.empty(n), np.empty((n, num_pes), dtype=np.complex128), np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32))

    def _hop_draw(self, name, num_pes, n, head, device_out):
        """a sample: a new ensemble of n trajectories, filled when this returns; head is what stands between num_pes and the flags"""
        state = self._hop_empty(int(num_pes), n, device_out)
        self._hop_call(name, num_pes, head, state, self._hop_pointers)
        if device_out:
            self.synchronize()
        return state

    @staticmethod
    def _hop_packet(model, n, trajectory_offset, seed, x0, p0, sigma_x, sigma_p, surface0):
        """n and the head of a sample from one packet"""
        n = int(n)
        if n < 1:
            raise ValueError("an ensemble has at least one trajectory")
        return n, (int(model), n, int(trajectory_offset), int(seed), float(x0), float(p0), float(sigma_x), float(sigma_p), int(surface0))

    @staticmethod
    def _hop_packets(model, n_per_group, trajectory_offset, seed, packets, surface0):
        """n and the head of a sample from a table of packets"""
        n_per_group, packets = int(n_per_group), _f64(packets)
        if packets.ndim != 2 or packets.shape[1] != 4 or packets.shape[0] < 1 or n_per_group < 1:
            raise ValueError("packets is (n_groups, 4) with n_groups >= 1, and a group has at least one trajectory")
        n_groups = packets.shape[0]
        return n_groups * n_per_group, (int(model), n_groups, n_per_group, int(trajectory_offset), int(seed), _ptr(packets), int(surface0))  # the pointer holds the table

    def _hop_sums(self, name, num_pes, head, state, pointers_of, width):
        """an observe: the sums on the side the ensemble is on, then on the host"""
        out = _like(state[0], width)
        (po,), _ = _io(out)
        self._hop_call(name, num_pes, head, state, pointers_of, tail=(po,))
        if _on_device(out):
            self.synchronize()
            return out.cpu().numpy()
        return out

    def _hop_sums_groups(self, name, num_pes, head, state, pointers_of, n_groups, width):
        """a grouped observe: the library brings the rows to the host itself"""
        out = np.empty((n_groups, width))
        self._hop_call(name, num_pes, head, state, pointers_of, tail=(_ptr(out),))
        return out

    def hop_sample(self, num_pes, model, n, seed, x0, p0, sigma_x, sigma_p, surface0=0, trajectory_offset=0, device_out=False):
        """gple_hop_sample: n trajectories drawn from the Gaussian (x0, sigma_x) x (p0, sigma_p) on the adiabatic surface surface0 -> the ensemble
        (x, p, b, surface, status).  device_out: tensors on the context's device (the call has completed when it returns)"""
        n, head = self._hop_packet(model, n, trajectory_offset, seed, x0, p0, sigma_x, sigma_p, surface0)
        return self._hop_draw("hop_sample", num_pes, n, head, device_out)

    @staticmethod
    def _hop_decoherence(decoherence):
        """the GPLE_HOP_DC_* of a name of HOP_DC_NAMES or of an integer"""
        if isinstance(decoherence, str):
            if decoherence not in HOP_DC_NAMES:
                raise ValueError(f"decoherence is None, an integer or one of {sorted(HOP_DC_NAMES)}")
            return HOP_DC_NAMES[decoherence]
        return int(decoherence)

    def hop_evolve(self, num_pes, model, state, seed, mass, dt, first_step, n_steps, x_left, x_right, reverse=False, trajectory_offset=0, decoherence=None,
                   edc_c=0.1):
        """gple_hop_evolve: the steps first_step ... first_step + n_steps - 1 of every running trajectory.  numpy: returns the evolved copy;
        device tensors: evolves the ensemble in place (asynchronously on the context's stream) and returns it.  reverse: GPLE_HOP_REVERSE.
        decoherence: None is gple_hop_evolve itself; "edc", "collapse_hop", "collapse_attempt" ("none", or a GPLE_HOP_DC_* integer) go through
        gple_hop_evolve_dc, the step with the decoherence correction 6a, edc_c (Hartree) being the constant of mode "edc" alone"""
        state, n = self._hop_own(num_pes, state)
        head = (int(model), n, int(trajectory_offset), int(seed), float(mass), float(dt), int(first_step), int(n_steps), float(x_left), float(x_right))
        self._hop_fssh_step("hop_evolve", num_pes, head, state, reverse, decoherence, edc_c)
        return state

    def _hop_fssh_step(self, name, num_pes, head, state, reverse, decoherence, edc_c, tail=()):
        """gple_<name>, or with a decoherence gple_<name>_dc, whose head ends in the mode and edc_c"""
        if decoherence is not None:
            name, head = name + "_dc", head + (self._hop_decoherence(decoherence), float(edc_c))
        self._hop_call(name, num_pes, head, state, self._hop_pointers, HOP_REVERSE if reverse else 0, tail)

    def hop_observe(self, num_pes, model, state, mass):
        """gple_hop_observe -> the 4 num_pes + 3 sums as a numpy array: counts [status][surface] (3 num_pes), sum |c_k|^2 (num_pes), sum x, sum p,
        sum (p^2 / 2 mass + E_surface).  With device tensors only these numbers cross"""
        state, n = self._hop_state(int(num_pes), state)
        return self._hop_sums("hop_observe", num_pes, (int(model), n, float(mass)), state, self._hop_pointers, 4 * int(num_pes) + 3)

    @staticmethod
    def _hop_grid(num_pes, grid):
        """the 6-tuple (x_first, dx, n_x, p_first, dp, n_p) of hop_bin with its types, and the length of its accumulator"""
        x_first, dx, n_x, p_first, dp, n_p = grid
        grid = (float(x_first), float(dx), int(n_x), float(p_first), float(dp), int(n_p))
        if grid[2] < 1 or grid[5] < 1:
            raise ValueError("a grid has at least one point per axis")
        return grid, (num_pes + num_pes * (num_pes - 1)) * grid[2] * grid[5] + 2

    @staticmethod
    def _hop_acc(acc, words):
        """acc of hop_bin / hop_density as (array or tensor, pointer, flags): int64 of `words` entries, numpy or contiguous on the GPU"""
        llp = C.POINTER(C.c_longlong)
        if _on_device(acc):
            if not acc.is_cuda or not acc.is_contiguous() or str(acc.dtype) != "torch.int64" or tuple(acc.shape) != (words,):
                raise ValueError(f"a device accumulator is a contiguous int64 tensor of {words} entries on the GPU")
            return acc, C.cast(acc.data_ptr(), llp), IO_DEVICE
        acc = np.ascontiguousarray(acc, dtype=np.int64)
        if acc.shape != (words,):
            raise ValueError(f"an accumulator has {words} entries")
        return acc, acc.ctypes.data_as(llp), 0

    def hop_bin(self, num_pes, model, state, grid, acc=None, bin_all=False):
        """gple_hop_bin: the ensemble added into the integer accumulator of grid = (x_first, dx, n_x, p_first, dp, n_p) -> acc, int64 of
        (num_pes + num_pes (num_pes - 1)) n_x n_p + 2 entries: the count planes per active surface, the (re, im) planes of 2^32 c_a conj(c_b)
        per pair a < b, then [binned, outside].  numpy arrays for a numpy ensemble, a tensor on the GPU for a device one.  acc=None starts from
        zero; a given acc is added to (GPLE_HOP_ACCUMULATE): numpy returns the sum as a copy, a tensor is added to in place (asynchronously on
        the context's stream) and returned.  bin_all: GPLE_HOP_BIN_ALL, finished trajectories too"""
        state, n = self._hop_state(int(num_pes), state)
        return self._hop_bin("hop_bin", int(num_pes), model, state, n, self._hop_pointers, grid, acc, bin_all)

    def _hop_bin(self, name, num_pes, model, state, n, pointers_of, grid, acc, bin_all):
        grid, words = self._hop_grid(num_pes, grid)
        flags = HOP_BIN_ALL if bin_all else 0
        if acc is None:
            acc = _like(state[0], words, np.int64)
        else:
            flags |= HOP_ACCUMULATE
            if _on_device(acc) != _on_device(state[0]):
                raise ValueError("the accumulator lives on the side the ensemble is on")
            if not _on_device(acc):
                acc = np.array(acc, dtype=np.int64)
        acc, pa, _ = self._hop_acc(acc, words)
        self._hop_call(name, num_pes, (int(model), n, *grid), state, pointers_of, flags, (pa,))
        return acc

    def hop_density(self, num_pes, grid, acc, n_norm):
        """gple_hop_density: the accumulator of hop_bin as the adiabatic density (num_pes, num_pes, n_x, n_p) complex, the phase.txt layout, on the
        side acc is on (a tensor: asynchronously on the context's stream); n_norm: the size of the whole ensemble"""
        return self._hop_density("hop_density", int(num_pes), grid, acc, n_norm)

    def _hop_density(self, name, num_pes, grid, acc, n_norm):
        grid, words = self._hop_grid(num_pes, grid)
        acc, pa, flags = self._hop_acc(acc, words)
        rho = _like(acc, (num_pes, num_pes, grid[2], grid[5]), np.complex128)
        (pr,), _ = _io(rho)
        self._check(getattr(self.lib, "gple_" + name)(self.ctx, num_pes, grid[2], grid[5], grid[1], grid[4], int(n_norm), flags, pa, pr))
        return rho

    # ---- grouped ensembles (gple_hop_*_groups; DESIGN.md §17, "A curve in one launch", driven by hopping.scan) --------------------------------
    # The same five arrays with n = n_groups n_per_group trajectories, trajectory i in group i / n_per_group; packets (n_groups, 4) rows
    # (x0, p0, sigma_x, sigma_p) and dt (n_groups,) are small numpy tables
    @staticmethod
    def _hop_groups(n, n_per_group):
        n_per_group = int(n_per_group)
        if n_per_group < 1 or n % n_per_group:
            raise ValueError("a grouped ensemble holds a whole number of groups of n_per_group >= 1 trajectories")
        return n // n_per_group, n_per_group

    @staticmethod
    def _hop_dt(dt, n_groups):
        dt = _f64(dt)
        if dt.shape != (n_groups,):
            raise ValueError("dt has one time step per group")
        return dt

    @staticmethod
    def _hop_hops(hops, n, dev):
        """the counters of a grouped step as (hops, pointer): None and a null pointer, a device tensor as it is, or a copy of a numpy array"""
        ip = C.POINTER(C.c_int)
        if hops is None:
            return None, None
        if _on_device(hops) != dev:
            raise ValueError("hops lives on the side the ensemble is on")
        if dev:
            if not hops.is_cuda or not hops.is_contiguous() or str(hops.dtype) != "torch.int32" or tuple(hops.shape) != (n, 2):
                raise ValueError("device hops is a contiguous int32 tensor of shape (n, 2) on the GPU")
            return hops, C.cast(hops.data_ptr(), ip)
        hops = np.array(hops, dtype=np.int32, order="C")
        if hops.shape != (n, 2):
            raise ValueError("hops has shape (n, 2)")
        return hops, hops.ctypes.data_as(ip)

    def hop_sample_groups(self, num_pes, model, n_per_group, seed, packets, surface0=0, trajectory_offset=0, device_out=False):
        """gple_hop_sample_groups: n_per_group trajectories per row (x0, p0, sigma_x, sigma_p) of packets -> the ensemble (x, p, b, surface,
        status) of len(packets) n_per_group trajectories.  A sigma may be 0: the coordinate is then the centre exactly.  device_out: tensors on
        the context's device (the call has completed when it returns)"""
        n, head = self._hop_packets(model, n_per_group, trajectory_offset, seed, packets, surface0)
        return self._hop_draw("hop_sample_groups", num_pes, n, head, device_out)

    def hop_evolve_groups(self, num_pes, model, state, n_per_group, seed, mass, dt, first_step, n_steps, x_left, x_right, reverse=False, trajectory_offset=0,
                          hops=None, decoherence=None, edc_c=0.1):
        """gple_hop_evolve_groups: the steps first_step ... first_step + n_steps - 1 of every running trajectory, group g with the time step
        dt[g].  numpy: returns the evolved copy; device tensors: evolves the ensemble in place (asynchronously on the context's stream) and
        returns it.  hops (None, or int32 (n, 2) on the side the ensemble is on): the hops taken and the frustrated hops of the call are added
        to it; the return value is then (state, hops), a numpy hops being a copy.  reverse: GPLE_HOP_REVERSE.  decoherence, edc_c: as hop_evolve
        (None is gple_hop_evolve_groups itself, anything else goes through gple_hop_evolve_groups_dc)"""
        state, n = self._hop_own(num_pes, state)
        n_groups, n_per_group = self._hop_groups(n, n_per_group)
        dt = self._hop_dt(dt, n_groups)
        hops, ph = self._hop_hops(hops, n, _on_device(state[0]))
        head = (int(model), n_groups, n_per_group, int(trajectory_offset), int(seed), float(mass), _ptr(dt), int(first_step), int(n_steps), float(x_left),
                float(x_right))
        self._hop_fssh_step("hop_evolve_groups", num_pes, head, state, reverse, decoherence, edc_c, (ph,))
        return state if hops is None else (state, hops)

    def hop_observe_groups(self, num_pes, model, state, n_per_group, mass):
        """gple_hop_observe_groups -> (n_groups, 4 num_pes + 3) numpy array, row g the sums of hop_observe over group g (the same bits).  With
        device tensors only these rows cross"""
        state, n = self._hop_state(int(num_pes), state)
        n_groups, n_per_group = self._hop_groups(n, n_per_group)
        return self._hop_sums_groups("hop_observe_groups", num_pes, (int(model), n_groups, n_per_group, float(mass)), state, self._hop_pointers, n_groups,
                                     4 * int(num_pes) + 3)

    # ---- Ehrenfest (mean-field) trajectories (gple_hop_*_mf; DESIGN.md §17, "Mean-field (Ehrenfest) trajectories") ------------------------------
    # The ensemble is the 5-tuple hop_sample returns.  A mean-field trajectory has no active surface: `surface` is never passed down and comes
    # back as the object it was
    @staticmethod
    def _hop_mf_pointers(state):
        """the pointers of x, p, b, status (no surface) and the io flags"""
        (px, pp, pb), flags = _io(*state[:3])
        ip = C.POINTER(C.c_int)
        return [px, pp, pb, C.cast(state[4].data_ptr(), ip) if flags else state[4].ctypes.data_as(ip)], flags

    def _hop_mf_state(self, num_pes, state, copy):
        """the checked ensemble with the caller's own surface object in it; copy: numpy x, p, b, status are copies (the evolve calls write them)"""
        checked, n = self._hop_state(int(num_pes), state)
        x, p, b, _, status = checked
        if copy and not _on_device(x):
            x, p, b, status = (np.array(a) for a in (x, p, b, status))
        return (x, p, b, state[3], status), n

    def _hop_step(self, name, num_pes, model, state, n, pointers_of, n_per_group, mass, dt, n_steps, x_left, x_right, extra=()):
        """the step of the methods that need no seed (_mf, _sqc, _mash): n_per_group None is the plain form, otherwise dt has a time step per
        group; extra ends the head"""
        if n_per_group is None:
            size, dt = (n,), float(dt)
        else:
            size = self._hop_groups(n, n_per_group)
            dt = _ptr(self._hop_dt(dt, size[0]))
        self._hop_call(name, num_pes, (int(model), *size, float(mass), dt, int(n_steps), float(x_left), float(x_right), *extra), state, pointers_of)
        return state

    def hop_evolve_mf(self, num_pes, model, state, mass, dt, n_steps, x_left, x_right):
        """gple_hop_evolve_mf: n_steps mean-field steps of every running trajectory (the force b^dagger Fd b, no hops, nothing random).  numpy:
        returns the evolved copy; device tensors: evolves the ensemble in place (asynchronously on the context's stream) and returns it"""
        state, n = self._hop_mf_state(num_pes, state, True)
        return self._hop_step("hop_evolve_mf", num_pes, model, state, n, self._hop_mf_pointers, None, mass, dt, n_steps, x_left, x_right)

    def hop_evolve_groups_mf(self, num_pes, model, state, n_per_group, mass, dt, n_steps, x_left, x_right):
        """gple_hop_evolve_groups_mf: hop_evolve_mf with the time step dt[g] for group g; a group's state has the bits hop_evolve_mf gives for
        that slice.  numpy: returns the evolved copy; device tensors: in place"""
        state, n = self._hop_mf_state(num_pes, state, True)
        return self._hop_step("hop_evolve_groups_mf", num_pes, model, state, n, self._hop_mf_pointers, n_per_group, mass, dt, n_steps, x_left, x_right)

    def hop_observe_mf(self, num_pes, model, state, mass):
        """gple_hop_observe_mf -> the 3 num_pes + 6 sums as a numpy array: weights [status][k] = sum |c_k|^2 over the trajectories of that status
        (3 num_pes), the counts per status (3), sum x, sum p, sum (p^2 / 2 mass + sum_k |c_k|^2 E_k).  With device tensors only these cross"""
        state, n = self._hop_mf_state(num_pes, state, False)
        return self._hop_sums("hop_observe_mf", num_pes, (int(model), n, float(mass)), state, self._hop_mf_pointers, 3 * int(num_pes) + 6)

    def hop_observe_groups_mf(self, num_pes, model, state, n_per_group, mass):
        """gple_hop_observe_groups_mf -> (n_groups, 3 num_pes + 6) numpy array, row g the sums of hop_observe_mf over group g (the same bits)"""
        state, n = self._hop_mf_state(num_pes, state, False)
        n_groups, n_per_group = self._hop_groups(n, n_per_group)
        return self._hop_sums_groups("hop_observe_groups_mf", num_pes, (int(model), n_groups, n_per_group, float(mass)), state, self._hop_mf_pointers, n_groups,
                                     3 * int(num_pes) + 6)

    def hop_bin_mf(self, num_pes, model, state, grid, acc=None, bin_all=False):
        """gple_hop_bin_mf: hop_bin from the amplitudes alone (the state's surface is ignored and never passed down) -> acc, int64 with the
        length and the plane order of hop_bin's: the first num_pes planes hold the sums of rint(2^32 |c_a|^2) and no counts, then the (re, im)
        planes of 2^32 c_a conj(c_b) per pair a < b, then [binned, outside].  acc and bin_all as hop_bin: numpy for a numpy ensemble, a tensor
        on the GPU for a device one; a given acc is added to (GPLE_HOP_ACCUMULATE), numpy as a copy, a tensor in place.  At most 2^31
        trajectories per call, and per accumulator"""
        state, n = self._hop_mf_state(num_pes, state, False)
        return self._hop_bin("hop_bin_mf", int(num_pes), model, state, n, self._hop_mf_pointers, grid, acc, bin_all)

    def hop_density_mf(self, num_pes, grid, acc, n_norm):
        """gple_hop_density_mf: the accumulator of hop_bin_mf as the adiabatic density (num_pes, num_pes, n_x, n_p) complex, the phase.txt
        layout, on the side acc is on (a tensor: asynchronously on the context's stream); n_norm: the size of the whole ensemble"""
        return self._hop_density("hop_density_mf", int(num_pes), grid, acc, n_norm)

    # ---- the smoothed density (gple_hop_smooth, gple_hop_smooth_mf; DESIGN.md §17, "The ensemble in phase space, smoothed") ------------------------
    def hop_smooth(self, num_pes, model, state, grid, bandwidth, n_norm, bin_all=False):
        """gple_hop_smooth: the ensemble as a Gaussian kernel density estimate on grid = (x_first, dx, n_x, p_first, dp, n_p) with
        bandwidth = (h_x, h_p) -> (rho, (used, nonfinite)).  rho is the adiabatic density (num_pes, num_pes, n_x, n_p) complex, the phase.txt
        layout, on the side the ensemble is on, as hop_density returns it: populations from the active surface, coherences from the amplitudes.
        The selection is hop_bin's (bin_all: GPLE_HOP_BIN_ALL); n_norm: the size of the whole ensemble.  The tallies are ready when this
        returns"""
        state, n = self._hop_state(int(num_pes), state)
        return self._hop_smooth("hop_smooth", int(num_pes), model, state, n, self._hop_pointers, grid, bandwidth, n_norm, bin_all)

    def hop_smooth_mf(self, num_pes, model, state, grid, bandwidth, n_norm, bin_all=False):
        """gple_hop_smooth_mf: hop_smooth from the amplitudes alone (the state's surface is ignored and never passed down), as hop_bin_mf and
        hop_density_mf -> (rho, (used, nonfinite))"""
        state, n = self._hop_mf_state(num_pes, state, False)
        return self._hop_smooth("hop_smooth_mf", int(num_pes), model, state, n, self._hop_mf_pointers, grid, bandwidth, n_norm, bin_all)

    def _hop_smooth(self, name, num_pes, model, state, n, pointers_of, grid, bandwidth, n_norm, bin_all):
        grid, _ = self._hop_grid(num_pes, grid)
        h_x, h_p = bandwidth
        rho = _like(state[0], (num_pes, num_pes, grid[2], grid[5]), np.complex128)
        (pr,), _ = _io(rho)
        tally = (C.c_longlong * 2)(0, 0)
        self._hop_call(name, num_pes, (int(model), n, *grid, float(h_x), float(h_p), int(n_norm)), state, pointers_of, HOP_BIN_ALL if bin_all else 0, (pr, tally))
        return rho, (int(tally[0]), int(tally[1]))

    # ---- symmetrical quasi-classical trajectories (gple_hop_*_sqc; DESIGN.md §17, "Symmetrical quasi-classical trajectories") ----------------------
    # The ensemble is the same 5-tuple; b holds the mapping amplitudes, which are not normalised.  The samples write surface (= surface0); the
    # evolve and observe calls never pass it down, as their _mf siblings
    @staticmethod
    def _hop_window(window, gamma):
        """(GPLE_HOP_WINDOW_*, gamma) of a name of HOP_WINDOW_NAMES or an integer; gamma None: the customary value of that window"""
        if isinstance(window, str):
            if window not in HOP_WINDOW_NAMES:
                raise ValueError(f"window is an integer or one of {sorted(HOP_WINDOW_NAMES)}")
            window = HOP_WINDOW_NAMES[window]
        window = int(window)
        if gamma is None:
            if window not in HOP_WINDOW_GAMMA:
                raise ValueError("no customary gamma for this window")
            gamma = HOP_WINDOW_GAMMA[window]
        return window, float(gamma)

    def hop_sample_sqc(self, num_pes, model, n, seed, x0, p0, sigma_x, sigma_p, surface0=0, window="triangle", gamma=None, trajectory_offset=0, device_out=False):
        """gple_hop_sample_sqc: x and p as hop_sample draws them (the same bits), the mapping amplitudes b on the start window of the adiabatic
        state surface0 ("square" or "triangle", gamma None: (sqrt(3) - 1) / 2 or 1 / 3) -> the ensemble (x, p, b, surface, status)"""
        window = self._hop_window(window, gamma)
        n, head = self._hop_packet(model, n, trajectory_offset, seed, x0, p0, sigma_x, sigma_p, surface0)
        return self._hop_draw("hop_sample_sqc", num_pes, n, head + window, device_out)

    def hop_sample_groups_sqc(self, num_pes, model, n_per_group, seed, packets, surface0=0, window="triangle", gamma=None, trajectory_offset=0, device_out=False):
        """gple_hop_sample_groups_sqc: hop_sample_sqc per row (x0, p0, sigma_x, sigma_p) of packets, as hop_sample_groups (a sigma may be 0)"""
        window = self._hop_window(window, gamma)
        n, head = self._hop_packets(model, n_per_group, trajectory_offset, seed, packets, surface0)
        return self._hop_draw("hop_sample_groups_sqc", num_pes, n, head + window, device_out)

    def hop_evolve_sqc(self, num_pes, model, state, mass, dt, n_steps, x_left, x_right, gamma):
        """gple_hop_evolve_sqc: n_steps steps of every running trajectory on the mapping Hamiltonian (the mean-field step with the force
        b^dagger Fd b - gamma tr Fd).  numpy: returns the evolved copy; device tensors: evolves the ensemble in place and returns it"""
        state, n = self._hop_mf_state(num_pes, state, True)
        return self._hop_step("hop_evolve_sqc", num_pes, model, state, n, self._hop_mf_pointers, None, mass, dt, n_steps, x_left, x_right, (float(gamma),))

    def hop_evolve_groups_sqc(self, num_pes, model, state, n_per_group, mass, dt, n_steps, x_left, x_right, gamma):
        """gple_hop_evolve_groups_sqc: hop_evolve_sqc with the time step dt[g] for group g; a group's state has the bits hop_evolve_sqc gives for
        that slice.  numpy: returns the evolved copy; device tensors: in place"""
        state, n = self._hop_mf_state(num_pes, state, True)
        return self._hop_step("hop_evolve_groups_sqc", num_pes, model, state, n, self._hop_mf_pointers, n_per_group, mass, dt, n_steps, x_left, x_right,
                              (float(gamma),))

    def hop_observe_sqc(self, num_pes, model, state, mass, window="triangle", gamma=None):
        """gple_hop_observe_sqc -> the 4 num_pes + 9 sums as a numpy array (hopping.unpack_sqc names them): the trajectories [status][window k],
        per status, per status in no window, sum e_k, sum x, sum p, sum H.  With device tensors only these cross"""
        state, n = self._hop_mf_state(num_pes, state, False)
        head = (int(model), n, float(mass), *self._hop_window(window, gamma))
        return self._hop_sums("hop_observe_sqc", num_pes, head, state, self._hop_mf_pointers, 4 * int(num_pes) + 9)

    def hop_observe_groups_sqc(self, num_pes, model, state, n_per_group, mass, window="triangle", gamma=None):
        """gple_hop_observe_groups_sqc -> (n_groups, 4 num_pes + 9) numpy array, row g the sums of hop_observe_sqc over group g (the same bits)"""
        state, n = self._hop_mf_state(num_pes, state, False)
        window = self._hop_window(window, gamma)
        n_groups, n_per_group = self._hop_groups(n, n_per_group)
        return self._hop_sums_groups("hop_observe_groups_sqc", num_pes, (int(model), n_groups, n_per_group, float(mass), *window), state, self._hop_mf_pointers,
                                     n_groups, 4 * int(num_pes) + 9)

    # ---- what left the box (gple_hop_outgoing*; DESIGN.md §17, "What left the box") ------------------------------------------------------------------
    # grid is (first, step, n_bins) of the momentum or the energy; acc is int64 of 2 num_pes n_bins + 4 entries: the planes [side][level][bin]
    # of weights times 2^32, then [binned, outside, running, unassigned] (hopping.outgoing_density reads it)
    def _hop_outgoing(self, name, num_pes, model, state, n, pointers_of, mass, grid, axis, acc, extra=()):
        first, step, n_bins = grid
        first, step, n_bins = float(first), float(step), int(n_bins)
        if n_bins < 1:
            raise ValueError("a grid has at least one point")
        if isinstance(axis, str):
            if axis not in HOP_AXIS_NAMES:
                raise ValueError(f"axis is an integer or one of {sorted(HOP_AXIS_NAMES)}")
            axis = HOP_AXIS_NAMES[axis]
        words, flags = 2 * num_pes * n_bins + 4, 0
        if acc is None:
            acc = _like(state[0], words, np.int64)
        else:
            flags = HOP_ACCUMULATE
            if _on_device(acc) != _on_device(state[0]):
                raise ValueError("the accumulator lives on the side the ensemble is on")
            if not _on_device(acc):
                acc = np.array(acc, dtype=np.int64)
        acc, pa, _ = self._hop_acc(acc, words)
        self._hop_call(name, num_pes, (int(model), n, float(mass), *extra, int(axis), first, step, n_bins), state, pointers_of, flags, (pa,))
        return acc

    def hop_outgoing(self, num_pes, model, state, mass, grid, axis="momentum", acc=None):
        """gple_hop_outgoing: the finished trajectories added to the plane of their channel (side, active surface) at the bin of their momentum
        (axis "momentum") or of p^2 / 2 mass + E_surface ("energy") on grid = (first, step, n_bins) -> acc.  numpy for a numpy ensemble, a
        tensor on the GPU for a device one; acc=None starts from zero, a given acc is added to (GPLE_HOP_ACCUMULATE): numpy returns the sum as a
        copy, a tensor is added to in place (asynchronously on the context's stream) and returned"""
        state, n = self._hop_state(int(num_pes), state)
        return self._hop_outgoing("hop_outgoing", int(num_pes), model, state, n, self._hop_pointers, mass, grid, axis, acc)

    def hop_outgoing_mf(self, num_pes, model, state, mass, grid, axis="momentum", acc=None):
        """gple_hop_outgoing_mf: hop_outgoing from the amplitudes alone: a finished trajectory adds rint(2^32 |c_k|^2) to every level k of its
        side, and its energy is p^2 / 2 mass + sum_k |c_k|^2 E_k.  The state's surface is never passed down.  At most 2^31 trajectories"""
        state, n = self._hop_mf_state(num_pes, state, False)
        return self._hop_outgoing("hop_outgoing_mf", int(num_pes), model, state, n, self._hop_mf_pointers, mass, grid, axis, acc)

    def hop_outgoing_sqc(self, num_pes, model, state, mass, grid, axis="momentum", window="triangle", gamma=None, acc=None):
        """gple_hop_outgoing_sqc: hop_outgoing with the level the window hop_observe_sqc finds for (window, gamma); a finished trajectory that
        no window holds is counted in `unassigned`.  The energy is H = p^2 / 2 mass + sum_k (e_k - gamma) E_k"""
        state, n = self._hop_mf_state(num_pes, state, False)
        return self._hop_outgoing("hop_outgoing_sqc", int(num_pes), model, state, n, self._hop_mf_pointers, mass, grid, axis, acc, self._hop_window(window, gamma))

    # ---- MASH trajectories (gple_hop_*_mash; DESIGN.md §17, "MASH trajectories") -------------------------------------------------------------------
    # The ensemble is the same 5-tuple, two levels only.  The samples draw amplitudes of their own; the step needs no seed, step counter or
    # offset; hop_observe and hop_observe_groups serve the ensemble unchanged
    def hop_sample_mash(self, num_pes, model, n, seed, x0, p0, sigma_x, sigma_p, surface0=0, trajectory_offset=0, device_out=False):
        """gple_hop_sample_mash: x and p as hop_sample draws them (the same bits), the amplitudes b with |S_z| drawn from the density 2 s on the
        side of the adiabatic state surface0 -> the ensemble (x, p, b, surface, status).  num_pes is 2"""
        n, head = self._hop_packet(model, n, trajectory_offset, seed, x0, p0, sigma_x, sigma_p, surface0)
        return self._hop_draw("hop_sample_mash", num_pes, n, head, device_out)

    def hop_sample_groups_mash(self, num_pes, model, n_per_group, seed, packets, surface0=0, trajectory_offset=0, device_out=False):
        """gple_hop_sample_groups_mash: hop_sample_mash per row (x0, p0, sigma_x, sigma_p) of packets, as hop_sample_groups (a sigma may be 0)"""
        n, head = self._hop_packets(model, n_per_group, trajectory_offset, seed, packets, surface0)
        return self._hop_draw("hop_sample_groups_mash", num_pes, n, head, device_out)

    def hop_evolve_mash(self, num_pes, model, state, mass, dt, n_steps, x_left, x_right):
        """gple_hop_evolve_mash: n_steps MASH steps of every running trajectory (the active surface follows the amplitudes; nothing random).
        numpy: returns the evolved copy; device tensors: evolves the ensemble in place (asynchronously on the context's stream) and returns it"""
        state, n = self._hop_own(num_pes, state)
        return self._hop_step("hop_evolve_mash", num_pes, model, state, n, self._hop_pointers, None, mass, dt, n_steps, x_left, x_right)

    def hop_evolve_groups_mash(self, num_pes, model, state, n_per_group, mass, dt, n_steps, x_left, x_right, hops=None):
        """gple_hop_evolve_groups_mash: hop_evolve_mash with the time step dt[g] for group g; a group's state has the bits hop_evolve_mash gives
        for that slice.  hops (None, or int32 (n, 2) on the side the ensemble is on): the hops taken and the frustrated hops of the call are
        added to it; the return value is then (state, hops), a numpy hops being a copy"""
        state, n = self._hop_own(num_pes, state)
        n_groups, n_per_group = self._hop_groups(n, n_per_group)
        dt = self._hop_dt(dt, n_groups)
        hops, ph = self._hop_hops(hops, n, _on_device(state[0]))
        head = (int(model), n_groups, n_per_group, float(mass), _ptr(dt), int(n_steps), float(x_left), float(x_right))
        self._hop_call("hop_evolve_groups_mash", num_pes, head, state, self._hop_pointers, tail=(ph,))
        return state if hops is None else (state, hops)

    # ---- reconstruction of a gridded density with the NLML GP (test/main_evolve.cpp; gple_nlml_weights / gple_grid_*) -------------------------
    SURVEY_FIELDS = ("max", "min", "weight", "argmax", "population", "potential", "kinetic")

    def _weights(self, fn, width, x, X, y):
        x = _f64(x)
        assert len(x) == width
        if not _on_device(X):
            X, y = _points(X), _f64(y)
        N = int(X.shape[0])
        b = _like(X, N)
        (pX, py, pb), flags = _io(X, y, b)
        self._check(fn(self.ctx, _ptr(x), pX, py, N, flags, pb))
        return b

    def nlml_weights(self, x, X, y):
        """gple_nlml_weights: b = K^-1 y of the NOCROSS kernel x = (w_d, w_g, a_x, a_p); numpy in -> numpy out, device tensors in -> device tensor out"""
        return self._weights(self.lib.gple_nlml_weights, 4, x, X, y)

    def nlml_cross_weights(self, x, X, y):
        """gple_nlml_cross_weights: the same for the cross-term kernel x = (w_d, w_g, a, c, b)"""
        return self._weights(self.lib.gple_nlml_cross_weights, 5, x, X, y)

    def grid_survey(self, num_pes, model, rho, x, p, mass, dx, dp):
        """gple_grid_survey: (num_pes^2, 8) per real plane q = row * num_pes + col: max, min, sum |v|, row-major index of the first maximum above 0
        (-1: none), and on diagonal planes population, potential and kinetic energy from the grid (SURVEY_FIELDS)"""
        rho, x, p = _rho(rho, num_pes), _axis(x), _axis(p)
        out = _like(rho, (num_pes * num_pes, 8))
        (pr, px, pp, po), flags = _io(rho, x, p, out)
        self._check(self.lib.gple_grid_survey(self.ctx, int(num_pes), int(model), pr, px, int(x.shape[0]), pp, int(p.shape[0]), float(mass), float(dx), float(dp),
                                              flags, po))
        return out

    def grid_select(self, num_pes, rho, x, p, q, n_select, seed, uniform=False):
        """gple_grid_select for plane q: (cells (n_select, 2) int32, X (n_select, 2), y (n_select,), K draws); device tensors in -> device tensors out"""
        rho, x, p = _rho(rho, num_pes), _axis(x), _axis(p)
        n_select = int(n_select)
        cells, X, y = _like(rho, (n_select, 2), np.int32), _like(rho, (n_select, 2)), _like(rho, n_select)
        (pr, px, pp, pc, pX, py), flags = _io(rho, x, p, cells, X, y)
        K = C.c_size_t(0)
        self._check(self.lib.gple_grid_select(self.ctx, int(num_pes), pr, px, int(x.shape[0]), pp, int(p.shape[0]), int(q), int(bool(uniform)), n_select, int(seed),
                                              flags, C.cast(pc, C.POINTER(C.c_int)), pX, py, C.byref(K)))
        return cells, X, y, K.value

    def _reconstruct(self, fn, plane_type, width, num_pes, model, rho, x, p, mass, dx, dp, planes, scale, want_pred):
        rho, x, p = _rho(rho, num_pes), _axis(x), _axis(p)
        nq = num_pes * num_pes
        if len(planes) != nq:
            raise ValueError("planes needs num_pes^2 entries")
        pred = _like(rho, (nq, int(x.shape[0]), int(p.shape[0]))) if want_pred else None
        sums = _like(rho, (nq, 6))
        arr, keep = (plane_type * nq)(), []
        for k, pl in enumerate(planes):
            if pl is None:
                continue
            xk, Xk, bk = pl
            if len(xk) != width:
                raise ValueError(f"a plane's kernel needs {width} hyper-parameters")
            if not _on_device(Xk):
                Xk, bk = _points(Xk), _f64(bk)
            (pX, pb, _), _ = _io(Xk, bk, rho)  # raises unless the plane's arrays live where rho does
            keep.append((Xk, bk))
            arr[k].x = (C.c_double * width)(*[float(v) for v in xk])
            arr[k].X, arr[k].b, arr[k].N = pX, pb, int(Xk.shape[0])
        sc = None if scale is None else _f64(scale)
        if sc is not None and sc.shape != (nq,):
            raise ValueError("scale needs num_pes^2 entries")
        (pr, px, pp, ppred, ps), flags = _io(rho, x, p, pred, sums)
        self._check(fn(self.ctx, int(num_pes), int(model), pr, px, int(x.shape[0]), pp, int(p.shape[0]), float(mass), float(dx), float(dp), arr, _ptr(sc), flags,
                       ppred, ps))
        return pred, sums

    def grid_reconstruct(self, num_pes, model, rho, x, p, mass, dx, dp, planes, scale=None, want_pred=True):
        """gple_grid_reconstruct: planes = num_pes^2 entries (x (4,), X (N, 2), b (N,)) or None (the plane is predicted as 0), on the side rho lives
        on; scale: num_pes^2 factors or None.  -> (pred (num_pes^2, nx, np) or None, sums (num_pes^2, 6): sum (c mu - v)^2, population, potential and
        kinetic energy of c mu on diagonal planes, sum (c mu)^2, sum c mu v)"""
        return self._reconstruct(self.lib.gple_grid_reconstruct, ReconPlane, 4, num_pes, model, rho, x, p, mass, dx, dp, planes, scale, want_pred)

    def grid_reconstruct_cross(self, num_pes, model, rho, x, p, mass, dx, dp, planes, scale=None, want_pred=True):
        """gple_grid_reconstruct_cross: the same with the cross-term kernel, x (5,) = (w_d, w_g, a, c, b) and b from nlml_cross_weights"""
        return self._reconstruct(self.lib.gple_grid_reconstruct_cross, ReconCrossPlane, 5, num_pes, model, rho, x, p, mass, dx, dp, planes, scale, want_pred)

    def evolve_n(self, num_pes, fits, model, mass, dt, density, new_points=False):
        """gple_evolve_n: one tick for an N-level system; fits and density in the packing order (0,0), (1,0), (1,1), (2,0), ...;
        density = {(i, j): (r (n, 2), rho (n,))} -> the same structure one tick later"""
        order = [(i, j) for i in range(num_pes) for j in range(i + 1)]
        empty = (np.zeros((0, 2)), np.zeros(0, dtype=complex))
        return self._tick("evolve_n", (int(num_pes),), order, [density.get(e, empty) for e in order], fits, model, mass, dt, new_points)

    def markov_chain(self, fit, num_steps, max_displacement, seed, r, want_chain=False):
        """Metropolis chains of all walkers on |cut-off prediction| of `fit`: (last points (n,2), acceptance ratio (n,)); with
        want_chain also the whole chains (num_steps + 1, n, 2)"""
        r = np.ascontiguousarray(np.asarray(r, dtype=np.float64).reshape(-1, 2)).copy()
        acc = np.empty(len(r))
        args = (self.ctx, self._elements([fit]), int(num_steps), float(max_displacement), int(seed), _ptr(r), len(r), _ptr(acc))
        if want_chain:
            chain = np.empty((int(num_steps) + 1, len(r), 2))
            self._check(self.lib.gple_markov_chain_trace(*args, _ptr(chain)))
            return r, acc, chain
        self._check(self.lib.gple_markov_chain(*args))
        return r, acc

    def cutoff_factor(self, prediction, variance):
        is_c = np.iscomplexobj(prediction)
        p = _cplx(prediction).view(np.float64) if is_c else _f64(prediction)
        var = _f64(variance)
        out = np.empty(len(var))
        self._check(self._fn("cutoff_factor")(*self._c(), _ptr(p), int(is_c), _ptr(var), len(var), *self._fl(), _ptr(out)))
        return out

    # ---- TrainingKernel / PredictiveKernel, TrainingComplexKernel / PredictiveComplexKernel ---------------------------------------------------
    def _fit(self, kind, theta, X, yy, y_is_complex, flags, defer_scalars):
        """yy: the labels as doubles; y_is_complex: the argument only gple_real_fit_create has, as a tuple (empty for the complex kernel)"""
        defer_scalars = defer_scalars and self.with_ctx  # the oracle computes everything at once
        theta, X = _f64(theta), _points(X)
        sc, h = (RealFitScalars if kind == "real" else ComplexFitScalars)(), C.c_void_p()
        self._check(self._fn(kind + "_fit_create")(*self._c(), _ptr(theta), _ptr(X), _ptr(yy), *y_is_complex, len(X), flags,
                                                   None if defer_scalars else C.byref(sc), C.byref(h)))
        return _Fit(self, h, kind, len(X), None if defer_scalars else scalars_to_dict(sc))

    def _predict(self, kind, fit, Xs, flags, labels, want):
        """labels, prediction and cutoff are M doubles for the real kernel and M (re, im) pairs for the complex one"""
        cplx = kind == "complex"
        Xs = _points(Xs)
        M = len(Xs)
        wide = 2 * M if cplx else M
        lab = None if labels is None else (_cplx(labels).view(np.float64) if cplx else _f64(labels))
        pred = np.empty(wide) if "prediction" in want else None
        var = np.empty(M) if "variance" in want else None
        cut = np.empty(wide) if "cutoff" in want else None
        ps = PredictScalars()
        self._check(self._fn(kind + "_predict")(*self._c(), fit.handle, _ptr(Xs), M, flags, _ptr(lab), _ptr(pred), _ptr(var), _ptr(cut), C.byref(ps)))
        d = scalars_to_dict(ps)
        if cplx:
            pred, cut = (None if a is None else a.view(np.complex128) for a in (pred, cut))
        else:
            d["error_derivative"] = d["error_derivative"][:4]
        d.update(prediction=pred, variance=var, cutoff=cut)
        return d

    def real_fit(self, theta, X, y, flags, defer_scalars=False):
        is_c = np.iscomplexobj(y)
        yy = _cplx(y).view(np.float64) if is_c else _f64(y)
        return self._fit("real", theta, X, yy, (int(is_c),), flags, defer_scalars)

    def real_predict(self, fit, Xs, flags=0, labels=None, want=("prediction", "variance", "cutoff")):
        return self._predict("real", fit, Xs, flags, labels, want)

    def complex_fit(self, theta, X, y, flags, defer_scalars=False):
        return self._fit("complex", theta, X, _cplx(y).view(np.float64), (), flags, defer_scalars)

    def complex_predict(self, fit, Xs, flags=0, labels=None, want=("prediction", "variance", "cutoff")):
        return self._predict("complex", fit, Xs, flags, labels, want)

    # ---- objective / NLML ------------------------------------------------------------------------------------
    def loose_function(self, x, X, y, X_extra, y_extra, want_grad=True):
        x, X, Xe = _f64(x), _points(X), _points(X_extra)
        yy, ye = _cplx(y).view(np.float64), _cplx(y_extra).view(np.float64)
        val = C.c_double()
        grad = np.empty(len(x)) if want_grad else None
        self._check(self._fn("loose_function")(*self._c(), _ptr(x), len(x), _ptr(X), _ptr(yy), len(X), _ptr(Xe), _ptr(ye),
                                               len(Xe), C.byref(val), _ptr(grad)))
        return val.value, grad

    def objective(self, X, y, X_extra, y_extra):
        """loose_function with its data resident on the device: returns f(x, want_grad=True) -> (value, grad or None).  The
        oracle has no device: there the closure simply keeps the arrays."""
        X, Xe = _points(X), _points(X_extra)
        yy, ye = _cplx(y), _cplx(y_extra)
        if not self.with_ctx:
            return lambda x, want_grad=True: self.loose_function(x, X, yy, Xe, ye, want_grad=want_grad)
        return _Objective(self, X, yy, Xe, ye)

    def nlml(self, x, X, y, want_grad=True):
        """len(x) == 4: (w_d, w_g, a_x, a_p), the NOCROSS build; len(x) == 5: (w_d, w_g, a, c, b), the lower-triangular ARD weight
        matrix of the default build of test/gpr.cpp"""
        x, X, y = _f64(x), _points(X), _f64(y)
        assert len(x) in (4, 5)
        val = C.c_double()
        grad = np.empty(len(x)) if want_grad else None
        self._check(self._fn("nlml" if len(x) == 4 else "nlml_cross")(*self._c(), _ptr(x), _ptr(X), _ptr(y), len(X), C.byref(val), _ptr(grad)))
        return val.value, grad

    def nlml_batch(self, xs, Xs, ys, want_grad=True, want_weights=False):
        """gple_nlml_batch: B problems in one launch; xs (B, 4) or (B, 5) hyper-parameters, Xs / ys lists of (N_b, 2) / (N_b,) arrays, or of device
        tensors (then every result is a device tensor).  -> (values (B,), grads (B, 4 or 5) or None, weights: list of (N_b,) or None, info (B,)
        int32: 0, or the 1-based column of the first non-positive pivot of a problem whose results are NaN)"""
        xs = np.atleast_2d(_f64(xs))
        B, width = xs.shape
        if width not in (4, 5) or len(Xs) != B or len(ys) != B:
            raise ValueError("xs must be (B, 4) or (B, 5), with one training set per row")
        dev = B > 0 and _on_device(Xs[0])
        if not dev:
            Xs, ys = [_points(X) for X in Xs], [_f64(y) for y in ys]
        ref = Xs[0] if dev else None
        values, info = _like(ref, B), _like(ref, B, np.int32)
        grads = _like(ref, (B, width)) if want_grad else None
        weights = [_like(ref, int(X.shape[0])) for X in Xs] if want_weights else None
        probs = (NlmlProblem * max(1, B))()
        flags = 0
        for b in range(B):
            (pX, py), flags = _io(Xs[b], ys[b])
            probs[b].x = (C.c_double * 5)(*xs[b], *([0.0] * (5 - width)))
            probs[b].X, probs[b].y, probs[b].N = pX, py, int(Xs[b].shape[0])
        wp = None
        if want_weights:
            wp = (_dp * max(1, B))(*[_io(w)[0][0] for w in weights])
        (pv, pg, pi), _ = _io(values, grads, info)
        self._check(self.lib.gple_nlml_batch(self.ctx, probs, B, int(width == 5), flags, pv, pg, wp, C.cast(pi, C.POINTER(C.c_int))))
        return values, grads, weights, info

    def nlml_fit_planes(self, planes, cross=False, options=None, want_weights=False):
        """gple_nlml_fit_planes: planes = list of (X (N, 2), y (N,), start, lower, upper), 4 (cross=False) or 5 values each; options: an OptOptions
        or None (the library's defaults).  -> (x (P, 4 or 5), f (P,), n_eval (P,) int, weights: list of (N,) or None)"""
        P, width = len(planes), 5 if cross else 4
        arr, keep = (NlmlFitPlane * max(1, P))(), []
        for q, (X, y, start, lower, upper) in enumerate(planes):
            X, y = _points(X), _f64(y)
            keep.append((X, y))
            arr[q].X, arr[q].y, arr[q].N = _ptr(X), _ptr(y), len(X)
            for name, v in (("start", start), ("lb", lower), ("ub", upper)):
                v = _f64(v)
                if v.shape != (width,):
                    raise ValueError(f"a plane needs {width} start values, lower and upper bounds")
                setattr(arr[q], name, (C.c_double * 5)(*v, *([0.0] * (5 - width))))
        x, f, ne = np.empty((P, 5)), np.empty(P), np.zeros(P, dtype=np.int32)
        weights = [np.empty(len(X)) for X, _ in keep] if want_weights else None
        wp = (_dp * max(1, P))(*[_ptr(w) for w in weights]) if want_weights else None
        self._check(self.lib.gple_nlml_fit_planes(self.ctx, arr, P, int(cross), None if options is None else C.byref(options), _ptr(x), _ptr(f),
                                                  ne.ctypes.data_as(C.POINTER(C.c_int)), wp))
        return x[:, :width].copy(), f, ne, weights

    def nlml_predict(self, x, X, y, Xs):
        x, X, y, Xs = _f64(x), _points(X), _f64(y), _points(Xs)
        assert len(x) in (4, 5)
        out = np.empty(len(Xs))
        self._check(self._fn("nlml_predict" if len(x) == 4 else "nlml_cross_predict")(*self._c(), _ptr(x), _ptr(X), _ptr(y), len(X), _ptr(Xs), len(Xs),
                                                                                       *self._fl(), _ptr(out)))
        return out
