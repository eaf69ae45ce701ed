"""Exact DVR wavepacket dynamics: the reference's schrodinger_equation/main.cpp, restated on the library's device entry points
(gple_dvr_hamiltonian, gple_dvr_propagate, gple_wigner; for the absorbing boundary gple_dvr_absorber, gple_dvr_propagator, gple_dvr_apply,
and gple_dvr_flux, gple_dvr_flux_apply for what the absorber took, gple_dvr_spectrum for its resolution in energy).

    setup()            main.cpp:41-146 with the defaults of schrodinger_equation/input.py
    initial_adiabatic_psi(), to_diabatic()  general.cpp:70-103 (Gaussian on the lowest adiabatic surface) taken to the diabatic basis (main.cpp:158-161)
    run()              the output loop of main.cpp:210-298: propagate, adiabatic psi, populations (general.cpp:480-495), <E> <x> <p> from psi
                       (general.cpp:443-478), the Wigner transform and its averages (general.cpp:324-411), the stop criteria (main.cpp:256-294)
    writers            x.txt, p.txt, t.txt, psi.txt, phase.txt, averages.txt in the reference's line layout; numbers as %g (output.py);
                       absorbed.txt (flux=True, no file of the reference's): t, the absorbed population per side and surface, what is left
                       spectrum.txt (spectrum=..., no file of the reference's): E, the absorbed population per unit energy per side and surface

The Hamiltonian is diagonalised once per run with numpy.linalg.eigh on the host (set-up, not the hot path: DESIGN.md §11).  The absorbing
boundary needs no eigh: the propagator of the output_step RK4 steps between two outputs is formed once on the device as a matrix power and
applied once per output.
"""
import math
import os
import time

import numpy as np

HBAR = 1.0                 # general.h:35
CHANGE_LIM = 1e-5  # general.h:46
PPL_LIM = 1e-4     # general.h:45 (the absorbing boundary only)
SAC, DAC, ECR, TSAC = 0, 1, 2, 3
REFLECTIVE, PERIODIC = 0, 1
ABSORBING = 2  # a constant of this driver only (general.h:88-93): the library's H is the reflective one plus gple_dvr_absorber
ABSORBER_C = math.sqrt(2.0) * 1.8540746773013719  # sqrt(2) K(1 / sqrt(2)) (pes.cpp:61)
RK4_ABSORBER_LIMIT = 2.0  # dt max W / hbar of the halving rule: [-2.5, 0] x [-0.7, 0.7] lies inside RK4's stability region


def cutoff(val):
    """The power of two <= val (general.cpp:33-36)."""
    return 2.0 ** int(math.floor(math.log2(val)))


def output_time_cutoff(x):
    """input.py's rounding of the output time to 1eN / 2eN / 5eN / 10eN (int() truncates towards zero, as there)."""
    logx = np.log10(x)
    n = int(logx)
    powx = np.power(10.0, n)
    resume = logx - n
    if resume < 0.3:
        return 2 * powx
    if resume < 0.7:
        return 5 * powx
    return 10 * powx


def absorbing_potential(x, mass, xmin, xmax, length):
    """absorbing_potential (pes.cpp:64-93) with x <= xmin on the left-hand branch, on the host: setup() sizes the time step with its maximum;
    the run takes W itself from gple_dvr_absorber."""
    x = np.asarray(x, dtype=np.float64)
    c = ABSORBER_C
    xi = c * np.where(x <= xmin, x - xmin, x - xmax) / length
    w = (2.0 * math.pi * HBAR / length) ** 2 * 2.0 / mass * (1.0 / (c - xi) ** 2 + 1.0 / (c + xi) ** 2 - 2.0 / c ** 2)
    return np.where((x > xmin) & (x < xmax), 0.0, w)


def setup(ln_energy=0.0, mass=2000.0, x0=-8.0, xmin=-15.0, xmax=15.0, dx_max=0.1, number_of_output=50, p0=None, sigma_p=None, output_time=None, dx=None,
          boundary=PERIODIC, dt_max=0.1):
    """The run's constants: input.py's defaults (p0 = sqrt(2 m e^lnE), sigma_p = p0 / 20, output time from the 1-2-5 rounding) then main.cpp:52-146.
    dx (optional) replaces the grid spacing main.cpp:74 derives (coarse grids for tests and probes).  boundary=ABSORBING adds the absorbing
    region on either side (main.cpp:79-95, 108) and the RK4 time step (main.cpp:130-135, dt_max: the input file's dt), halved until
    dt max W / hbar <= RK4_ABSORBER_LIMIT (the reference bounds the kinetic term only): dt is the step the run takes, dt_rule the reference's,
    halvings how often it was halved; the step counts are doubled along, so the output times stay."""
    if p0 is None:
        p0 = float(np.sqrt(2.0 * mass * np.exp(ln_energy)))
    if sigma_p is None:
        sigma_p = p0 / 20.0
    if output_time is None:
        output_time = float(output_time_cutoff((-x0 - x0) / (p0 / mass) / number_of_output))
    sigma_x = HBAR / 2.0 / sigma_p                                   # main.cpp:59
    p0max = p0 + 3.0 * sigma_p                                       # main.cpp:66
    if dx is None:
        dx = cutoff(min(dx_max, 2 * math.pi * HBAR / p0max / 5.0))   # main.cpp:74
    n_grids = int((xmax - xmin) / dx) + 1                            # main.cpp:76, 95 (no absorbing region)
    if boundary == ABSORBING:
        return _setup_absorbing(mass, x0, p0, sigma_p, sigma_x, xmin, xmax, dx, n_grids, output_time, dt_max)
    pmin, pmax = p0 - math.pi * HBAR / dx / 2.0, p0 + math.pi * HBAR / dx / 2.0  # main.cpp:103-104
    i = np.arange(n_grids)
    x = xmin + dx * i                                                # main.cpp:108
    p = ((n_grids - 1 - i) * pmin + i * pmax) / (n_grids - 1)        # main.cpp:109
    total_time = (xmax - xmin) / (p0 / mass) * 2.0                   # main.cpp:127
    dt = output_time                                                 # main.cpp:130-140 (no absorbing boundary)
    return dict(mass=mass, x0=x0, p0=p0, sigma_p=sigma_p, sigma_x=sigma_x, xmin=xmin, xmax=xmax, dx=dx, n_grids=n_grids, x=x, p=p,
                total_time=total_time, output_time=output_time, dt=dt, total_step=int(total_time / dt), output_step=int(output_time / dt))


def _setup_absorbing(mass, x0, p0, sigma_p, sigma_x, xmin, xmax, dx, interior, output_time, dt_max):
    length = 2 * math.pi * HBAR / (p0 - 3.0 * sigma_p)               # main.cpp:79-89
    n_abs = int(length / dx)                                         # main.cpp:93
    n_grids = interior + 2 * n_abs                                   # main.cpp:95
    pmin, pmax = p0 - math.pi * HBAR / dx / 2.0, p0 + math.pi * HBAR / dx / 2.0
    i = np.arange(n_grids)
    x = xmin + dx * (i - n_abs)                                      # main.cpp:108
    p = ((n_grids - 1 - i) * pmin + i * pmax) / (n_grids - 1)
    total_time = (xmax - xmin) / (p0 / mass) * 2.0
    dt_rule = cutoff(min(dt_max, HBAR / 500.0 / (sigma_p * p0 / mass)))  # main.cpp:134
    total_step, output_step = int(total_time / dt_rule), int(output_time / dt_rule)  # main.cpp:144-145
    w_max = float(absorbing_potential(x, mass, xmin, xmax, length).max())
    dt, halvings = dt_rule, 0
    while dt * w_max / HBAR > RK4_ABSORBER_LIMIT:
        dt, halvings, total_step, output_step = dt / 2.0, halvings + 1, 2 * total_step, 2 * output_step
    return dict(mass=mass, x0=x0, p0=p0, sigma_p=sigma_p, sigma_x=sigma_x, xmin=xmin, xmax=xmax, dx=dx, n_grids=n_grids, x=x, p=p, total_time=total_time,
                output_time=output_time, dt=dt, total_step=total_step, output_step=output_step, absorbing_length=length, n_absorbing=n_abs, dt_rule=dt_rule,
                halvings=halvings, w_max=w_max)


def initial_adiabatic_psi(x, x0, p0, sigma_x, num_pes):
    """wavefunction_initialization (general.cpp:75-104): a Gaussian on the lowest surface, normalised on the grid."""
    n = len(x)
    dx = (x[n - 1] - x[0]) / (n - 1)
    psi = np.zeros(num_pes * n, dtype=np.complex128)
    psi[:n] = np.exp(-((x - x0) / 2 / sigma_x) ** 2 + 1j * (p0 * x / HBAR)) / math.sqrt(math.sqrt(2.0 * math.pi) * sigma_x)
    psi[:n] /= math.sqrt(np.vdot(psi, psi).real * dx)
    return psi


def to_diabatic(psi_adia, basis):
    """psi_dia[j n + a] = sum_k C_a(j, k) psi_adia[k n + a] (main.cpp:160-161, pes.cpp:96-120)."""
    n, num_pes = basis.shape[0], basis.shape[1]
    return np.einsum("ajk,...ka->...ja", basis, psi_adia.reshape(psi_adia.shape[:-1] + (num_pes, n))).reshape(psi_adia.shape)


def to_adiabatic(psi_dia, basis):
    """psi_adia = basis^T psi_dia per grid point (main.cpp:221)."""
    n, num_pes = basis.shape[0], basis.shape[1]
    return np.einsum("ajk,...ja->...ka", basis, psi_dia.reshape(psi_dia.shape[:-1] + (num_pes, n))).reshape(psi_dia.shape)


def derivative_matrix(n, dx):
    """The first-derivative DVR matrix of general.cpp:417-436 on one surface: (-1)^(j-k) / dx / (j - k) off the diagonal."""
    j = np.arange(n)
    d = j[:, None] - j[None, :]
    with np.errstate(divide="ignore"):
        D = np.where(d == 0, 0.0, np.where(d % 2 == 0, 1.0, -1.0) / dx / np.where(d == 0, 1, d))
    return D


def populations(psi_adia, n, dx, num_pes):
    """calculate_population (general.cpp:480-495)."""
    return np.array([np.vdot(psi_adia[m * n:(m + 1) * n], psi_adia[m * n:(m + 1) * n]).real * dx for m in range(num_pes)])


def psi_averages(psi_dia, H, D, x, dx, num_pes):
    """calculate_average (general.cpp:443-478): <E> = psi^H H psi dx, <x> = sum x |psi|^2 dx, <p> = psi^H (-i hbar D) psi dx."""
    n = len(x)
    E = np.vdot(psi_dia, H @ psi_dia).real * dx
    X = float(sum(np.dot(x, np.abs(psi_dia[m * n:(m + 1) * n]) ** 2) for m in range(num_pes))) * dx
    Dpsi = np.concatenate([D @ psi_dia[m * n:(m + 1) * n] for m in range(num_pes)])
    P = np.vdot(psi_dia, -1j * HBAR * Dpsi).real * dx
    return E, X, P


def fmt(v):
    return "%g" % v


def write_grid(path, values):
    """x.txt / p.txt / t.txt: one number per line (main.cpp:112-121, 219)."""
    with open(path, "w") as f:
        f.write("".join(fmt(v) + "\n" for v in values))


def psi_line(psi_adia):
    """output_grided_population (general.cpp:281-288): ' |psi_i|^2' for every entry, then a newline."""
    return "".join(" " + fmt(v) for v in (psi_adia * np.conj(psi_adia)).real) + "\n"


def phase_block(P):
    """One output time of phase.txt (general.cpp:384-409): a line per element (i, j) row-major with ' re im' per (x, p), p fastest, then a
    blank line.  P: (num_pes, num_pes, n, n_p) complex."""
    num_pes = P.shape[0]
    lines = []
    for i in range(num_pes):
        for j in range(num_pes):
            v = P[i, j].reshape(-1)
            pairs = np.empty(2 * len(v))
            pairs[0::2], pairs[1::2] = v.real, v.imag
            lines.append("".join(" " + fmt(u) for u in pairs) + "\n")
    return "".join(lines) + "\n"


def phase_text(api, P):
    """phase_block of every output time of P (T, num_pes, num_pes, n, n_p), on either side, converted on the device by gple_format_g: the same
    bytes in one call (a line per element, an empty line per output time)"""
    num_pes, n, n_p = int(P.shape[-3]), int(P.shape[-2]), int(P.shape[-1])
    return api.format_g(P, 2 * n * n_p, num_pes * num_pes)


def averages_line(t, E, X, P, pops, phase_avg):
    """One line of averages.txt (main.cpp:245-253): t <E> <x> <p> populations <E> <x> <p> of the Wigner function."""
    return " ".join(fmt(v) for v in [t, E, X, P, *pops, *phase_avg]) + "\n"


def spectrum_levels(end_time, dt):
    """The smallest J with 2^J dt >= end_time: the 2^J steps of the spectrum's transform cover the run."""
    J = 0
    while 2 ** J * dt < end_time:
        J += 1
    return J


def spectrum_energies(s, adiabatic_energies, n_E):
    """The default energies of run(spectrum=n_E): n_E momenta uniform in p0 +- 3 sigma_p (p0 itself for n_E = 1) as total energies in H's own
    zero, E = p^2 / 2m + the lowest adiabatic energy at the grid point nearest x0.  adiabatic_energies: (n, num_pes) of gple_dvr_hamiltonian."""
    n_E = int(n_E)
    if n_E < 1:
        raise ValueError("spectrum needs at least one energy")
    p = np.linspace(s["p0"] - 3.0 * s["sigma_p"], s["p0"] + 3.0 * s["sigma_p"], n_E) if n_E > 1 else np.array([s["p0"]])
    lowest = float(np.min(np.asarray(adiabatic_energies)[int(np.argmin(np.abs(s["x"] - s["x0"])))]))
    return p ** 2 / 2.0 / s["mass"] + lowest


def run(api, model=DAC, num_pes=2, boundary=PERIODIC, ln_energy=0.0, out_dir=None, write_phase="text", max_outputs=None, chunk_bytes=1 << 30,
        p_grid=None, log=None, flux=False, until_absorbed=False, spectrum=None, **setup_kw):
    """The loop of main.cpp:210-298.  boundary=ABSORBING: no eigh; the propagator of output_step RK4 steps is formed once (gple_dvr_propagator, kept
    on the device) and applied once per output (gple_dvr_apply); the Wigner transform is the reflective one (general.cpp:363-364), <E> uses the
    real H, and the stop criteria carry the PplLim clause.  write_phase: "text" (phase.txt), "npy" (phase_<k>.npy per output time) or None;
    out_dir None writes no file.  max_outputs caps the output times.  Returns a dict with the setup, per-output records and the final stdout line.
    flux (absorbing boundary only): U comes with the quadratic forms of gple_dvr_flux, one per side of the box (the grid points left and right
    of its centre) and adiabatic surface; before every application of U the state's figures (gple_dvr_flux_apply, times dx) join a running
    total, so every record carries `absorbed` (2, num_pes): what has left up to its output time, [left | right][surface], reflection and
    transmission for a packet that starts on the left.  The figures and the populations left add up to the initial population to rounding;
    a figure may be slightly negative.  absorbed.txt has a line per output: t, the 2 num_pes figures, the population left; the
    result gains `absorbed`, `scattering_line` (the final line's head, the figures, the remainder) and `flux_seconds`.
    until_absorbed (absorbing boundary only): the PplLim clause is the only stop, tested at every output whatever <x> is.
    spectrum (absorbing boundary only): a number n_E of energies (spectrum_energies) or an array of total energies in H's own zero.  After the
    loop one gple_dvr_spectrum call resolves what the absorber took in energy, over 2^J steps from psi0 with J = spectrum_levels(the run's end
    time, dt): rho_c(E) = dx dt / (2 pi hbar) psi_e^H D_c psi_e, a population per unit energy per side and surface, not clamped.
    spectrum.txt has a line per energy: E, the 2 num_pes figures; the result gains `spectrum` (n_E, 1 + 2 num_pes: those lines),
    `spectrum_levels`, `spectrum_remaining` (the population after the 2^J steps) and `spectrum_seconds`."""
    absorbing = boundary == ABSORBING
    if (flux or until_absorbed) and not absorbing:
        raise ValueError("flux and until_absorbed belong to boundary=ABSORBING")
    if spectrum is not None and (not absorbing or isinstance(spectrum, bool)):
        raise ValueError("spectrum (a number of energies or an array of them) belongs to boundary=ABSORBING")
    if absorbing:
        setup_kw["boundary"], boundary = ABSORBING, REFLECTIVE  # H and the Wigner transform of the reflective boundary (the reference's switches fall through)
    s = setup(ln_energy, **setup_kw)
    n, dx, x, mass = s["n_grids"], s["dx"], s["x"], s["mass"]
    p = s["p"] if p_grid is None else np.asarray(p_grid, dtype=np.float64)
    say = log or (lambda *_: None)
    t0 = time.perf_counter()
    H, energies, basis = api.dvr_hamiltonian(num_pes, model, boundary, x[0], dx, n, mass)
    t_h = time.perf_counter()
    if absorbing:
        if s["output_step"] < 1:
            raise ValueError("the output time is shorter than one time step")
        W = api.dvr_absorber(x[0], dx, n, mass, s["xmin"], s["xmax"], s["absorbing_length"])
        n_left = int(np.sum(x < (s["xmin"] + s["xmax"]) / 2.0))
        if flux:
            U, G = api.dvr_flux(num_pes, n, H, W, s["dt"], s["output_step"], basis, n_left, device_out=True)
        else:
            U = api.dvr_propagator(num_pes, n, H, W, s["dt"], s["output_step"], device_out=True)
        t_eigh, t_power = 0.0, time.perf_counter() - t_h
        say(f"dx = {dx:g}, {n} grids from {x[0]:g} to {x[-1]:g}; dt = {s['dt']:g} ({s['halvings']} halvings), {s['total_step']} steps; "
            f"propagator of {s['output_step']} steps, {num_pes * n} x {num_pes * n}: {t_power:.2f} s")
    else:
        eigval, eigvec = np.linalg.eigh(H)
        t_eigh, t_power = time.perf_counter() - t_h, 0.0
        say(f"dx = {dx:g}, {n} grids from {x[0]:g} to {x[-1]:g}; dt = {s['dt']:g}, {s['total_step']} steps; eigh of {num_pes * n} x {num_pes * n}: {t_eigh:.2f} s")
    psi0 = to_diabatic(initial_adiabatic_psi(x, s["x0"], s["p0"], s["sigma_x"], num_pes), basis)
    D = derivative_matrix(n, dx)
    steps = list(range(0, s["total_step"] + 1, s["output_step"]))  # iStep % OutputStep == 0 (main.cpp:217); total_step runs to 1e9 after halvings
    if max_outputs is not None:
        steps = steps[:max_outputs]
    per_time = 16 * num_pes * num_pes * n * len(p) + 64 * num_pes * n
    chunk = max(1, min(64, int(chunk_bytes // per_time)))
    files = {}
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        write_grid(os.path.join(out_dir, "x.txt"), x)
        write_grid(os.path.join(out_dir, "p.txt"), p)
        for name in ("t.txt", "psi.txt", "averages.txt") + (("absorbed.txt",) if flux else ()):
            files[name] = open(os.path.join(out_dir, name), "w")
        if write_phase == "text":
            files["phase.txt"] = open(os.path.join(out_dir, "phase.txt"), "wb")
    # phase.txt on the device: P stays there and only its text crosses; an api without format_g keeps the Python writer
    device_text = bool(files) and write_phase == "text" and hasattr(api, "format_g")
    records, stop, last_x, old_pop, pops = [], None, s["x0"], np.zeros(num_pes), None
    absorbed = np.zeros((2, num_pes))  # what has left before the current output
    t_loop = time.perf_counter()
    try:
        for c0 in range(0, len(steps), chunk):
            times = np.array([k * s["dt"] for k in steps[c0:c0 + chunk]])
            if absorbing:  # the chunk's states from the last one; the first output is psi0 itself
                first = psi0[None, :] if c0 == 0 else np.empty((0, len(psi0)), dtype=np.complex128)
                psi_dia = np.concatenate([first, api.dvr_apply(num_pes, n, U, psi0 if c0 == 0 else psi_dia[-1], len(times) - len(first))])
            else:
                psi_dia = api.dvr_propagate(num_pes, n, eigvec, eigval, psi0, times)
            psi_adia = to_adiabatic(psi_dia, basis)
            if flux:
                leaving = api.dvr_flux_apply(num_pes, n, G, psi_dia) * dx  # what each state of the chunk loses to the next application of U
            if device_text:
                P, wav = api.wigner(num_pes, boundary, x[0], dx, p, psi_adia, energies=energies, mass=mass, averages=True, device_out=True)
            else:
                P, wav = api.wigner(num_pes, boundary, x[0], dx, p, psi_adia, energies=energies, mass=mass, phase=write_phase is not None, averages=True)
            written = 0
            for q, t in enumerate(times):
                pops = populations(psi_adia[q], n, dx, num_pes)
                E, X, Pm = psi_averages(psi_dia[q], H, D, x, dx, num_pes)
                records.append(dict(t=t, E=E, x=X, p=Pm, populations=pops, phase_averages=wav[q].copy()))
                if flux:
                    records[-1]["absorbed"] = absorbed.copy()
                    if files:
                        files["absorbed.txt"].write(" ".join(fmt(v) for v in [t, *absorbed.ravel(), float(np.sum(pops))]) + "\n")
                    absorbed += leaving[q]
                if files:
                    files["t.txt"].write(fmt(t) + "\n")
                    files["psi.txt"].write(psi_line(psi_adia[q]))
                    files["averages.txt"].write(averages_line(t, E, X, Pm, pops, wav[q]))
                    written = q + 1
                    if write_phase == "text" and not device_text:
                        files["phase.txt"].write(phase_block(P[q]).encode())
                    elif write_phase == "npy":
                        np.save(os.path.join(out_dir, f"phase_{len(records) - 1}.npy"), P[q])
                if until_absorbed:
                    if float(np.sum(pops)) < PPL_LIM:
                        stop = f"ALMOST ALL POPULATION HAVE BEEN ABSORBED, STOP EVOLVING AT {t:g}"
                        break
                elif X > 0.0:  # main.cpp:256-287
                    if X > -s["x0"]:
                        stop = f"GET OUT OF INTERACTING REGION, STOP EVOLVING AT {t:g}"
                    elif (X - last_x) * s["p0"] < 0:
                        stop = f"DIRECTION REVERSED DUE TO REFLECTION / PBC, STOP EVOLVING AT {t:g}"
                    elif absorbing and float(np.sum(pops)) < PPL_LIM:
                        stop = f"ALMOST ALL POPULATION HAVE BEEN ABSORBED, STOP EVOLVING AT {t:g}"
                    elif np.all(np.abs(pops - old_pop) < CHANGE_LIM):
                        stop = f"POPULATION ON EACH PES IS STABLE. STOP EVOLVING AT {t:g}"
                    if stop:
                        break
                last_x, old_pop = X, pops
            if device_text and written:
                files["phase.txt"].write(phase_text(api, P[:written]))  # the chunk's output times up to a stop, in one call
            if stop:
                break
    finally:
        for f in files.values():
            f.close()
    t_end = time.perf_counter()
    head = math.log(s["p0"] ** 2 / 2.0 / mass) if model == DAC else s["p0"]  # main.cpp:308-321
    final_line = " ".join(fmt(v) for v in [head, *pops])
    say(stop or "FINISHED ALL OUTPUT TIMES")
    extra = {}
    if flux:
        taken = records[-1]["absorbed"] if records else np.zeros((2, num_pes))
        extra = dict(absorbed=taken, scattering_line=" ".join(fmt(v) for v in [head, *taken.ravel(), float(np.sum(pops))]), flux_seconds=t_power)
    if spectrum is not None:
        t_s = time.perf_counter()
        E = spectrum_energies(s, energies, spectrum) if isinstance(spectrum, (int, np.integer)) else np.atleast_1d(np.asarray(spectrum, dtype=np.float64))
        levels = spectrum_levels(records[-1]["t"] if records else 0.0, s["dt"])
        if levels > 30:
            raise ValueError("the run is longer than 2^30 time steps")
        density, _, left = api.dvr_spectrum(num_pes, n, H, W, s["dt"], levels, basis, n_left, psi0, E)
        rows = np.concatenate([E[:, None], np.asarray(density).reshape(len(E), 2 * num_pes) * (dx * s["dt"] / (2.0 * math.pi * HBAR))], axis=1)
        if out_dir is not None:
            with open(os.path.join(out_dir, "spectrum.txt"), "wb") as f:
                if hasattr(api, "format_g"):
                    f.write(api.format_g(rows, rows.shape[1], join=True))
                else:
                    f.write("".join(" ".join(fmt(v) for v in row) + "\n" for row in rows).encode())
        extra.update(spectrum=rows, spectrum_levels=levels, spectrum_remaining=left * dx, spectrum_seconds=time.perf_counter() - t_s)
        say(f"spectrum of {len(E)} energies over 2^{levels} steps: {extra['spectrum_seconds']:.2f} s")
    return dict(**extra, setup=s, records=records, stop=stop, final_line=final_line, eigh_seconds=t_eigh, propagator_seconds=t_power, total_seconds=t_end - t0,
                seconds_per_output=(t_end - t_loop) / max(1, len(records)), stop_time=records[-1]["t"] if records else None)
