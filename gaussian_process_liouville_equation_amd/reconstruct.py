"""Reconstruction of an exact phase-space density with the NLML GP: the loop body of the reference's test/main_evolve.cpp:56-179 for one
state, on the library's device entry points (gple_grid_survey, gple_grid_select, gple_nlml, gple_nlml_weights, gple_grid_reconstruct;
DESIGN.md §13), for either build of the reference's kernel: kernel="nocross", the diagonal ARD weights (w_d, w_g, a_x, a_p), or
kernel="cross", the default build's lower-triangular weight matrix W = [[a, 0], [c, b]] with (w_d, w_g, a, c, b) (gple_nlml_cross,
gple_nlml_cross_weights, gple_grid_reconstruct_cross).

    set_initial_value()           gpr.cpp:113-195: bounds and start values of the hyper-parameters (w_d, w_g, a_x, a_p) of every plane
    is_small()                    gpr.cpp:197-210 on the survey's max / min
    optimize()                    gpr.cpp:535-643: Nelder-Mead on the NLML value, then one projected-BFGS pass on value + gradient
    population_from_gpr() ...     gpr.cpp:715-911 (both branches), host numpy on b = K^-1 y
    obey_conservation()           gpr.cpp:913-992: the factors of the diagonal planes
    reconstruct()                 survey -> is_small -> select -> optimise -> weights -> reconstruct -> obey_conservation -> reconstruct(scale)
    run_mqcl()                    the exact MQCLE run of exact_mqcl.run with a reconstruction at every output time; log.txt, choose.txt, sim.txt
    read_grid(), phase_blocks()   read_coord (test/io.cpp:11-23) and the output times of a phase.txt, one block of bytes at a time
    run_files()                   main_evolve.cpp / main_screenshot.cpp on a directory an exact solver wrote: phase.txt read back on the device
                                  (gple_parse_g)

The state is num_pes^2 real planes (SuperMatrix, test/io.cpp:25-72): plane q = row * num_pes + col is Re rho_ii, Re rho_ij (row < col) or
Im rho_ij (row > col)."""
import math
import mmap
import os
import time

import numpy as np

from . import _capi, exact_mqcl
from .exact import DAC, fmt

SMALL = 1e-2                       # is_very_small_everywhere, gpr.cpp:200
DIAG_MIN, DIAG_MAX = 1e-8, 1e-5    # gpr.cpp:138-139
GAUSS_MIN, GAUSS_MAX = 1e-4, 1.0   # gpr.cpp:140-141
XTOL_ABS, INITIAL_STEP = 1e-10, 0.5  # gpr.cpp:592-596
DBL_MAX = float(np.finfo(np.float64).max)
KERNELS = {"nocross": 4, "cross": 5}  # hyper-parameters per plane


def _width(kernel):
    if kernel not in KERNELS:
        raise ValueError('kernel must be "nocross" or "cross"')
    return KERNELS[kernel]


class State:
    """What stays the same from one output time to the next: the grid, the model, dx and dp as the experiment defines them
    ((x[nx - 1] - x[0]) / nx, main_evolve.cpp:23) and the device copies of the grid for states that live on the device"""

    def __init__(self, api, num_pes, model, x, p, mass):
        self.num_pes, self.model, self.mass = int(num_pes), int(model), float(mass)
        self.x, self.p = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(p, dtype=np.float64)
        self.dx, self.dp = (self.x[-1] - self.x[0]) / len(self.x), (self.p[-1] - self.p[0]) / len(self.p)
        self._dev = None

    def grid_like(self, rho):
        """(x, p) on the side rho lives on"""
        if not hasattr(rho, "data_ptr"):
            return self.x, self.p
        if self._dev is None:
            import torch
            self._dev = (torch.from_numpy(self.x).to(rho.device), torch.from_numpy(self.p).to(rho.device))
        return self._dev


def _host(api, a):
    """a result on the host; device results are complete once the context's stream has drained (the library's calls with device pointers are
    asynchronous on its own stream, which torch's copies do not wait for)"""
    if not hasattr(a, "data_ptr"):
        return np.asarray(a)
    api.synchronize()
    return a.cpu().numpy()


def is_small(survey):
    """gpr.cpp:197-210: max < 1e-2 and min > -1e-2, per plane"""
    return (survey[:, 0] < SMALL) & (survey[:, 1] > -SMALL)


def set_initial_value(survey, x, p, num_pes, kernel="nocross"):
    """gpr.cpp:113-195 -> (lower, upper, start), each (num_pes^2, 4) in the order (w_d, w_g, a_x, a_p): sigma_p = p[argmax of plane 0] / 20,
    sigma_x = 0.5 / sigma_p; the ARD weights start at the inverse widths and are bounded below by the inverse box lengths, unbounded above.
    kernel="cross": (num_pes^2, 5) in the order (w_d, w_g, a, c, b), a and b as a_x and a_p, the cross weight c starts at 0 and is unbounded
    both ways (gpr.cpp:143-145, 176-181: its slot keeps the vectors' initial values)"""
    cross = _width(kernel) == 5
    arg = int(survey[0, 3])
    if arg < 0:
        raise ValueError("plane (0, 0) has no value above 0: the reference's start values are undefined there (gpr.cpp:119-136)")
    sigma_p = p[arg % len(p)] / 20.0
    sigma_x = 0.5 / sigma_p
    nq = num_pes * num_pes
    lower = np.tile([DIAG_MIN, GAUSS_MIN, 1.0 / (x.max() - x.min()), 1.0 / (p.max() - p.min())], (nq, 1))
    upper = np.tile([DIAG_MAX, GAUSS_MAX, DBL_MAX, DBL_MAX], (nq, 1))
    start = np.tile([DIAG_MIN, GAUSS_MAX, 1.0 / sigma_x, 1.0 / sigma_p], (nq, 1))
    if cross:
        lower, upper, start = (np.insert(a, 3, v, axis=1) for a, v in ((lower, -DBL_MAX), (upper, DBL_MAX), (start, 0.0)))
    return lower, upper, start


def _options(maxeval):
    # NLopt with set_xtol_abs alone (gpr.cpp:592-596): every other tolerance off
    return _capi.OptOptions(0.0, 0.0, XTOL_ABS, 0.0, INITIAL_STEP, int(maxeval or 0))


def optimize(api, X, y, start, lower, upper, maxeval=0):
    """gpr.cpp:535-643 for one plane: the library's Nelder-Mead on the NLML value, then its augmented-Lagrangian search without constraints
    (one projected-BFGS pass) on value + gradient, from the first search's minimiser.  gple_nlml keeps the reference's half gradient on the two
    kernel weights (gpr.cpp:425, 432): they are doubled here.  Five start values run the same on gple_nlml_cross (Api.nlml chooses by length).
    -> (hyper-parameters, NLML there, evaluations)"""
    count = [0]

    def value(xs, want_grad):
        count[0] += 1
        v, g = api.nlml(np.array(xs), X, y, want_grad=want_grad)
        if not math.isfinite(v):
            v = DBL_MAX
        if g is not None:
            g = np.where(np.isfinite(g), g, 0.0)
            g[:2] *= 2.0
        return v, g

    opt = _options(maxeval)
    xv, _, _ = _capi.minimize_neldermead(api.lib, lambda xs: value(xs, False)[0], start, lower, upper, options=opt)
    xv, _, _ = _capi.minimize_auglag_eq(api.lib, value, lambda xs, want_grad: ((), ()), 0, xv, lower, upper, options=opt)
    xv = np.array(xv)
    return xv, value(xv, False)[0], count[0]  # "Best Combination": the value once more at the result (gpr.cpp:633)


def optimize_planes(api, sets, starts, lowers, uppers, maxeval=0):
    """optimize for several planes at once on gple_nlml_fit_planes: sets = [(X, y), ...] with at most _capi.NLML_BATCH_MAX_N points
    each; the searches run in lock-step inside the library and every round of evaluations is one launch.  Each plane's result is that of the same
    search on that plane alone.  -> (hyper-parameters (P, 4 or 5), NLML there (P,), evaluations (P,), weights K^-1 y at the result: list of (N,))"""
    cross = len(starts[0]) == 5
    planes = [(X, y, start, lower, upper) for (X, y), start, lower, upper in zip(sets, starts, lowers, uppers)]
    return api.nlml_fit_planes(planes, cross=cross, options=_options(maxeval), want_weights=True)


def population_from_gpr(hyper, b):
    """gpr.cpp:715-762: (2 pi)^Dim w_g^2 / (product of the weight matrix's diagonal) sum b, Dim = 1 — a_x a_p, or a b of the five
    cross-term parameters (:750)"""
    return 2.0 * math.pi * hyper[1] ** 2 / (hyper[2] * hyper[-1]) * float(np.sum(b))


def kinetic_energy_from_gpr(hyper, X, b, mass):
    """gpr.cpp:853-911: the same coefficient times sum (P_i^2 + a_p^-2) b_i / 2 mass; with five parameters (W W^T)^-1_pp = 1 / b^2 (:896),
    the same expression on the last parameter"""
    return 2.0 * math.pi * hyper[1] ** 2 / (hyper[2] * hyper[-1]) * float(np.dot(X[:, 1] ** 2 + hyper[-1] ** -2, b)) / 2.0 / mass


def potential_energy_from_gpr(api, num_pes, model, level, hyper, X, b, step_divisor=16):
    """gpr.cpp:765-841: the integral of E_level(x) rho(x) with rho(x) = w_g^2 sqrt(2 pi) / a_p sum b_i exp(-(a_x (x - X_i))^2 / 2).  The reference
    integrates with Boost's Bulirsch-Stoer after x = (1 - t) / t; here: the trapezoid rule on a uniform grid of step 1 / (step_divisor a_x) — never
    above 1 / step_divisor, so that a kernel much wider than the potential's features does not under-sample the energy — over
    [min X - 40 / a_x, max X + 40 / a_x], beyond which every term is below exp(-800).  The rule converges geometrically for this integrand.
    Five parameters (w_d, w_g, a, c, b), gpr.cpp:801-806 as the text reads: it takes Characteristic(0, 1), the zero ABOVE the diagonal of the
    lower-triangular matrix generate_kernels fills (:313-321), where the cross weight c = Characteristic(1, 0) is meant, so its marginal is
    w_g^2 sqrt(2 pi) / |b| exp(-(a (x - X_i))^2 / 2) — the expression above with a_p = |b| — and not the kernel's true marginal
    w_g^2 sqrt(2 pi / (b^2 + c^2)) exp(-a^2 b^2 (x - X_i)^2 / (2 (b^2 + c^2))).  Kept as the reference has it."""
    ax = float(hyper[2])
    h = min(1.0 / (step_divisor * ax), 1.0 / step_divisor)
    lo, hi = float(X[:, 0].min()) - 40.0 / ax, float(X[:, 0].max()) + 40.0 / ax
    n = int(math.ceil((hi - lo) / h)) + 1
    # blocks of 8192 grid points, and of those only the ones within 40 / a_x of a point (one grid point to spare): everywhere else every term is
    # exp(-800) = 0 exactly, so leaving a block out leaves the sum as it is, bit for bit.  A fit that ends with a huge a_x (a search that
    # failed: 1e12 has been seen) has 1e13 grid points but only two blocks per point; neither the grid nor the energies are held as a whole.
    first = np.floor((X[:, 0] - 40.0 / ax - lo) / h).astype(np.int64) - 1
    last = np.ceil((X[:, 0] + 40.0 / ax - lo) / h).astype(np.int64) + 1
    blocks = sorted({int(k) for f, l in zip(first, last) for k in range(max(0, int(f)) // 8192, min(n - 1, int(l)) // 8192 + 1)})
    total = 0.0
    for i0 in (8192 * k for k in blocks):  # bounded memory: 8192 x N exponentials at a time
        xs = lo + h * np.arange(i0, min(n, i0 + 8192))
        energy = api.pes_adiabatic_n(num_pes, model, xs)[0][:, level]
        d = ax * (xs[:, None] - X[None, :, 0])
        total += float(np.dot(energy, np.exp(-0.5 * d * d) @ b))
    ap = hyper[3] if len(hyper) == 4 else abs(hyper[4])  # sqrt(2 pi / b^2)
    return hyper[1] ** 2 * math.sqrt(2.0 * math.pi) / ap * total * h


def obey_conservation(population, energy, small_diag, initial_energy):
    """gpr.cpp:913-992 on the from-parameters population and energy of the diagonal planes (arrays over the levels; small_diag: the levels
    that are 0 everywhere): one level -> 1 / population; more -> the 2 x 2 system [sum population; sum energy] of the first half and the second
    half of the non-small levels = [1; initial energy].  -> (factor per level, singular); a singular system leaves every factor at 1"""
    levels = [i for i in range(len(population)) if not small_diag[i]]
    factors = np.ones(len(population))
    if not levels:
        return factors, False
    if len(levels) == 1:
        if population[levels[0]] == 0.0 or not math.isfinite(population[levels[0]]):
            return factors, True
        factors[levels[0]] = 1.0 / population[levels[0]]
        return factors, False
    half = len(levels) // 2
    A = np.zeros((2, 2))
    for k, i in enumerate(levels):
        A[0, 0 if k < half else 1] += population[i]
        A[1, 0 if k < half else 1] += energy[i]
    det = A[0, 0] * A[1, 1] - A[0, 1] * A[1, 0]
    if not np.all(np.isfinite(A)) or abs(det) <= 1e-14 * (abs(A[0, 0] * A[1, 1]) + abs(A[0, 1] * A[1, 0])):
        return factors, True
    c = np.linalg.solve(A, np.array([1.0, initial_energy]))
    for k, i in enumerate(levels):
        factors[i] = c[0 if k < half else 1]
    return factors, False


FITS = ("serial", "batched")


def reconstruct(api, state, rho, n_points=200, seed=0, maxeval=0, start=None, initial_energy=None, keep_pred=False, log=None, kernel="nocross",
                fit="serial"):
    """One pass of main_evolve.cpp:56-179 on the adiabatic state rho ((num_pes, num_pes, nx, np) complex; numpy, or a torch tensor on the
    GPU, which then never leaves it).  start: the previous output time's hyper-parameters (main_evolve.cpp:94), default set_initial_value;
    initial_energy: the conserved energy (main_evolve.cpp:48), default this state's own; maxeval caps each of the two searches (0: the
    library's defaults); kernel: "nocross" (four hyper-parameters per plane) or "cross" (five, the reference's default build).  Returns the
    record of log.txt and more: nlml, hyper (nq, 4 or 5), mse_before / mse_after (nq), factors (nq), singular,
    is_small (nq), per level exact / grid / gpr population, potential and kinetic energy before and after, features / labels / cells per
    plane, draws, sums_before / sums_after (nq, 6), seconds per phase, and with keep_pred the two predictions (nq, nx, np) on the host.
    fit: "serial" searches plane after plane with optimize; "batched" searches all live planes at once with optimize_planes, which also hands over
    their weights (planes of more than _capi.NLML_BATCH_MAX_N points still go through optimize)."""
    if fit not in FITS:
        raise ValueError('fit must be "serial" or "batched"')
    num_pes, model, mass, dx, dp = state.num_pes, state.model, state.mass, state.dx, state.dp
    width = _width(kernel)
    nlml_weights, grid_reconstruct = (api.nlml_weights, api.grid_reconstruct) if width == 4 else (api.nlml_cross_weights, api.grid_reconstruct_cross)
    nq = num_pes * num_pes
    x, p = state.grid_like(rho)
    say = log or (lambda *_: None)
    clock = {}
    t0 = time.perf_counter()
    survey = _host(api, api.grid_survey(num_pes, model, rho, x, p, mass, dx, dp))
    small = is_small(survey)
    lower, upper, first = set_initial_value(survey, state.x, state.p, num_pes, kernel)
    hyper = np.array(first if start is None else start, dtype=np.float64).reshape(nq, width).copy()
    diag = [i * num_pes + i for i in range(num_pes)]
    exact = {"population": survey[diag, 4], "potential": survey[diag, 5], "kinetic": survey[diag, 6]}
    if initial_energy is None:
        initial_energy = float(exact["potential"].sum() + exact["kinetic"].sum())
    clock["survey"] = time.perf_counter() - t0

    t0 = time.perf_counter()
    chosen = [api.grid_select(num_pes, rho, x, p, q, n_points, seed, uniform=bool(small[q])) for q in range(nq)]
    cells, features, labels = [_host(api, c[0]) for c in chosen], [_host(api, c[1]) for c in chosen], [_host(api, c[2]) for c in chosen]
    draws = [c[3] for c in chosen]
    clock["select"] = time.perf_counter() - t0

    t0 = time.perf_counter()
    nlml, evals = 0.0, 0
    live = [q for q in range(nq) if not small[q]]  # "0 everywhere": no optimisation, the hyper-parameters stay (gpr.cpp:575-579)
    together = [q for q in live if fit == "batched" and len(features[q]) <= _capi.NLML_BATCH_MAX_N]
    found = {}
    if together:
        hs, values, ns, ws = optimize_planes(api, [(features[q], labels[q]) for q in together], hyper[together], lower[together], upper[together], maxeval)
        found = {q: (hs[k], float(values[k]), int(ns[k]), ws[k]) for k, q in enumerate(together)}
    for q in live:
        if q not in found:
            found[q] = optimize(api, features[q], labels[q], hyper[q], lower[q], upper[q], maxeval) + (None,)
        hyper[q], value, n = found[q][:3]
        nlml, evals = nlml + value, evals + n
        say(f"  plane {q}: NLML {value:.6g} at {np.array2string(hyper[q], precision=5)} after {n} evaluations")
    clock["optimize"] = time.perf_counter() - t0

    t0 = time.perf_counter()
    weights = [None if small[q] else found[q][3] if found[q][3] is not None else nlml_weights(hyper[q], features[q], labels[q]) for q in range(nq)]
    on_device = hasattr(rho, "data_ptr")

    def planes():
        out = []
        for q in range(nq):
            if small[q]:
                out.append(None)
                continue
            Xq, bq = features[q], weights[q]
            if on_device:
                import torch
                Xq, bq = torch.from_numpy(Xq).to(rho.device), torch.from_numpy(bq).to(rho.device)
            out.append((hyper[q], Xq, bq))
        return out

    plane_args = planes()
    pred_b, sums_b = grid_reconstruct(num_pes, model, rho, x, p, mass, dx, dp, plane_args, None, want_pred=keep_pred)
    sums_b = _host(api, sums_b)

    def from_gpr():
        pop, pot, kin = np.zeros(num_pes), np.zeros(num_pes), np.zeros(num_pes)
        for i, q in enumerate(diag):
            if small[q]:
                continue
            pop[i] = population_from_gpr(hyper[q], weights[q])
            pot[i] = potential_energy_from_gpr(api, num_pes, model, i, hyper[q], features[q], weights[q])
            kin[i] = kinetic_energy_from_gpr(hyper[q], features[q], weights[q], mass)
        return pop, pot, kin

    pop_b, pot_b, kin_b = from_gpr()
    level_factor, singular = obey_conservation(pop_b, pot_b + kin_b, small[diag], initial_energy)
    factors = np.ones(nq)
    factors[diag] = level_factor
    # The scaled labels' weights are K^-1 (c y) = c K^-1 y (gpr.cpp:952-955, 986-989) and the three numbers are linear in them, so the factor
    # is applied to the numbers: summing c b_i afresh would round each product, an error of eps sum |b_i|, which a fit with w_d at its lower
    # bound (a Gram matrix of condition 1e16, weights of 1e6 and more that cancel) lifts above the 1e-10 the two constraints are solved to.
    pop_a, pot_a, kin_a = level_factor * pop_b, level_factor * pot_b, level_factor * kin_b
    pred_a, sums_a = grid_reconstruct(num_pes, model, rho, x, p, mass, dx, dp, plane_args, factors, want_pred=keep_pred)
    sums_a = _host(api, sums_a)
    clock["reconstruct"] = time.perf_counter() - t0

    rec = dict(nlml=nlml, hyper=hyper, evaluations=evals, is_small=small, factors=factors, singular=singular, initial_energy=initial_energy,
               mse_before=sums_b[:, 0].copy(), mse_after=sums_a[:, 0].copy(), sums_before=sums_b, sums_after=sums_a, survey=survey,
               cells=cells, features=features, labels=[labels[q] * factors[q] for q in range(nq)], draws=draws, seconds=clock)
    for name, ex, gb, ga, k in (("population", exact["population"], pop_b, pop_a, 1), ("potential", exact["potential"], pot_b, pot_a, 2),
                                ("kinetic", exact["kinetic"], kin_b, kin_a, 3)):
        rec[f"{name}_exact"] = ex
        rec[f"{name}_grid_before"], rec[f"{name}_grid_after"] = sums_b[diag, k], sums_a[diag, k]
        rec[f"{name}_gpr_before"], rec[f"{name}_gpr_after"] = gb, ga
    if keep_pred:
        rec["pred_before"], rec["pred_after"] = _host(api, pred_b), _host(api, pred_a)
    return rec


def log_line(t, rec):
    """One line of log.txt (main_evolve.cpp:135-178): t, NLML sum, the hyper-parameters (four or five per plane), per plane MSE without / with the constraints, per level
    exact / grid / parameters population, potential and kinetic energy without and with the constraints"""
    v = [t, rec["nlml"], *rec["hyper"].ravel()]
    for q in range(len(rec["mse_before"])):
        v += [rec["mse_before"][q], rec["mse_after"][q]]
    for i in range(len(rec["population_exact"])):
        for name in ("population", "potential", "kinetic"):
            v += [rec[f"{name}_exact"][i], rec[f"{name}_grid_before"][i], rec[f"{name}_gpr_before"][i], rec[f"{name}_grid_after"][i], rec[f"{name}_gpr_after"][i]]
    return " ".join("%.16g" % a for a in v) + "\n"


def choose_block(rec):
    """print_point (io.cpp:74-92): per plane one line ' x p x p ...', then an empty line"""
    return "".join("".join(f" {fmt(a)} {fmt(b)}" for a, b in f) + "\n" for f in rec["features"]) + "\n"


def sim_block(pred):
    """main_evolve.cpp:145-160: per plane one line of the nx * np predicted values, then an empty line"""
    return "".join("".join(" " + fmt(v) for v in plane.ravel()) + "\n" for plane in pred) + "\n"


def _open_outputs(out_dir, write_sim):
    if out_dir is None:
        return {}
    os.makedirs(out_dir, exist_ok=True)
    return {name: open(os.path.join(out_dir, name), "w") for name in ("log.txt", "choose.txt") + (("sim.txt",) if write_sim else ())}


def _write_record(files, t, rec, write_sim):
    if files:
        files["log.txt"].write(log_line(t, rec))
        files["choose.txt"].write(choose_block(rec))
        if write_sim:
            files["sim.txt"].write(sim_block(rec["pred_after"]))
    rec.pop("pred_before", None), rec.pop("pred_after", None)


def _say_record(say, t, rec):
    say(f"T = {t:g}: NLML {rec['nlml']:.6g}, MSE {np.array2string(rec['mse_before'], precision=3)} -> {np.array2string(rec['mse_after'], precision=3)}, "
        + ", ".join(f"{k} {1e3 * v:.1f} ms" for k, v in rec["seconds"].items()))


def run_mqcl(api, out_dir=None, model=DAC, num_pes=2, ln_energy=0.0, n_points=200, seed=0, maxeval=0, write_sim=False, max_outputs=None, log=None,
             kernel="nocross", fit="serial", **setup_kw):
    """The exact MQCLE run of exact_mqcl.run with the reconstruction of main_evolve.cpp at every output time.  Each output's state is moved to
    the device once and the four reconstruction entry points work on that resident copy.  Writes log.txt, choose.txt and (write_sim) sim.txt
    in the reference's layouts next to exact_mqcl.run's files (phase.txt is not written: it is what this run replaces).  kernel: "nocross" or
    "cross", and fit: "serial" or "batched", as in reconstruct.  Returns exact_mqcl.run's
    dict with the reconstruction records under "reconstructions"."""
    import torch
    say = log or (lambda *_: None)
    _width(kernel)
    if fit not in FITS:
        raise ValueError('fit must be "serial" or "batched"')
    files, recs, carry = _open_outputs(out_dir, write_sim), [], {}

    def on_output(t, adia):
        if "state" not in carry:
            s = exact_mqcl.setup(ln_energy, **setup_kw)
            carry["state"] = State(api, num_pes, model, s["x"], s["p"], s["mass"])
        dev = torch.from_numpy(np.ascontiguousarray(adia)).cuda()
        rec = reconstruct(api, carry["state"], dev, n_points=n_points, seed=seed + len(recs), maxeval=maxeval, start=carry.get("hyper"),
                          initial_energy=carry.get("energy"), keep_pred=write_sim, log=log, kernel=kernel, fit=fit)
        carry["hyper"] = rec["hyper"]
        carry.setdefault("energy", rec["initial_energy"])
        rec["t"] = t
        _say_record(say, t, rec)
        _write_record(files, t, rec, write_sim)
        recs.append(rec)

    try:
        res = exact_mqcl.run(api, model=model, num_pes=num_pes, ln_energy=ln_energy, out_dir=out_dir, write_phase=None, max_outputs=max_outputs, log=log,
                             on_output=on_output, **setup_kw)
    finally:
        for f in files.values():
            f.close()
    res["reconstructions"] = recs
    return res


def read_grid(path):
    """read_coord (test/io.cpp:11-23): every number of x.txt / p.txt / t.txt, wherever the line breaks are (a few KB: read on the host)"""
    with open(path, "rb") as f:
        return np.array([float(token) for token in f.read().split()], dtype=np.float64)


def phase_blocks(path, num_pes, nx, np_, outputs=None):
    """The output times of a phase.txt, in file order: each block's bytes (a bytearray: num_pes^2 lines and the empty line behind them).  The
    host finds a block's end in the mapped file without converting anything — the next empty line at or behind the least that
    2 nx np num_pes^2 numbers can take — and reads that block alone: memory is one block, never the file.  outputs: the indices to yield
    (default: all); the others are stepped over unread, and the search stops behind the last one.  ValueError with the output's index where
    the file ends inside a block or a block does not have num_pes^2 lines."""
    nq = num_pes * num_pes
    least = nq * (2 * 2 * nx * np_ + 1)  # a blank and a digit per number, a newline per line
    wanted = None if outputs is None else set(outputs)
    last = None if wanted is None else max(wanted, default=-1)
    if os.path.getsize(path) == 0:
        return
    with open(path, "rb") as f, mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as m:
        at, index = 0, 0
        while at < len(m) and (last is None or index <= last):
            end = m.find(b"\n\n", min(len(m), at + least - 1))
            if end < 0:
                if m[at:].strip():
                    raise ValueError(f"phase.txt ends inside output {index}")
                return  # a few blank bytes behind the last block
            end += 2
            if wanted is None or index in wanted:
                newlines, found = 0, m.find(b"\n", at, end)
                while found >= 0 and newlines <= nq + 1:
                    newlines, found = newlines + 1, m.find(b"\n", found + 1, end)
                if newlines != nq + 1:
                    raise ValueError(f"output {index} of phase.txt does not have {nq} lines before its empty line")
                block = bytearray(end - at)
                f.seek(at)
                f.readinto(block)
                yield block
            at, index = end, index + 1


def _parse_host(block):
    """Api.parse_g's result for an api without it: float() per token, and the lines that hold one"""
    data = bytes(block)
    return np.array([float(token) for token in data.split()], dtype=np.float64), sum(1 for line in data.split(b"\n") if line.strip())


def run_files(api, in_dir, out_dir=None, model=DAC, num_pes=2, mass=2000.0, n_points=200, seed=0, maxeval=0, outputs=None, write_sim=False,
              kernel="nocross", fit="serial", log=None):
    """main_evolve.cpp:16-179 on a directory that exact.run or exact_mqcl.run (write_phase="text") or one of the reference's solvers wrote: reads
    x.txt, p.txt and t.txt, then for every output time of phase.txt uploads the block's bytes, converts them on the device (Api.parse_g, DESIGN.md
    §15) and reconstructs the state where it lies — it never visits the host.  Each output starts from the previous one's hyper-parameters
    (main_evolve.cpp:94), the conserved energy is that of the first output reconstructed (:48) and output `index` draws with seed + index: the
    carry of run_mqcl.  outputs: the indices into t.txt to reconstruct (default: all; a single one is main_screenshot.cpp); the others are
    never uploaded, and a selected output starts from the last selected one before it.  Both triangles of the state are converted and, as in
    reconstruct, only the upper one is used: read_density's averaging with the element below the diagonal is not restated.  An
    api without parse_g takes the host route, float() per token into a numpy state.  Writes log.txt, choose.txt and (write_sim) sim.txt into
    out_dir; returns the list of records (each with its "t" and "index").  ValueError naming the output where a block does not hold
    2 nx np num_pes^2 numbers in num_pes^2 lines, or phase.txt has fewer outputs than asked for."""
    say = log or (lambda *_: None)
    _width(kernel)
    if fit not in FITS:
        raise ValueError('fit must be "serial" or "batched"')
    x, p, t = (read_grid(os.path.join(in_dir, name)) for name in ("x.txt", "p.txt", "t.txt"))
    nx, n_p, nq = len(x), len(p), num_pes * num_pes
    indices = list(range(len(t))) if outputs is None else sorted({int(i) for i in outputs})
    if indices and not 0 <= indices[0] <= indices[-1] < len(t):
        raise ValueError(f"outputs must be indices into t.txt (0 .. {len(t) - 1})")
    state = State(api, num_pes, model, x, p, mass)
    on_device = hasattr(api, "parse_g")
    files, recs, hyper, energy = _open_outputs(out_dir, write_sim), [], None, None
    try:
        blocks = phase_blocks(os.path.join(in_dir, "phase.txt"), num_pes, nx, n_p, outputs=indices)
        for index, block in zip(indices, blocks):
            t0 = time.perf_counter()
            values, lines = api.parse_g(block, device_out=True) if on_device else _parse_host(block)
            if len(values) != 2 * nx * n_p * nq or lines != nq:
                raise ValueError(f"output {index} of phase.txt holds {len(values)} numbers in {lines} lines, not {2 * nx * n_p * nq} in {nq}")
            if on_device:
                import torch
                rho = torch.view_as_complex(values.view(num_pes, num_pes, nx, n_p, 2))
            else:
                rho = values.view(np.complex128).reshape(num_pes, num_pes, nx, n_p)
            t_read = time.perf_counter() - t0
            rec = reconstruct(api, state, rho, n_points=n_points, seed=seed + index, maxeval=maxeval, start=hyper, initial_energy=energy,
                              keep_pred=write_sim, log=log, kernel=kernel, fit=fit)
            hyper, energy = rec["hyper"], rec["initial_energy"]
            rec["t"], rec["index"] = float(t[index]), index
            rec["seconds"] = {"read": t_read, **rec["seconds"]}
            _say_record(say, t[index], rec)
            _write_record(files, t[index], rec, write_sim)
            recs.append(rec)
    finally:
        for f in files.values():
            f.close()
    if len(recs) != len(indices):
        raise ValueError(f"phase.txt ends before output {indices[len(recs)]}")
    return recs
