"""Exact MQCLE phase-space dynamics: the reference's liouville_equation/main.cpp restated on the library's device entry points
(gple_mqcl_transform, gple_mqcl_evolve, gple_mqcl_observe).

    setup()            main.cpp:41-116 with the defaults of schrodinger_equation/input.py (liouville_equation/ reads the same input file)
    initial_density()  density_matrix_initialization (general.cpp:68-106): a Gaussian in rho_00 of the adiabatic basis, normalised on the grid
    run()              the output loop of main.cpp:117-337: evolve OutputStep steps, observe, write, the stop criterion of :302, the final line
    writers            x.txt, p.txt, t.txt, phase.txt, averages.txt in the reference's line layout; numbers as %g (exact.py)
"""
import math
import os
import time

import numpy as np

from .exact import DAC, HBAR, cutoff, fmt, output_time_cutoff, phase_block, phase_text, write_grid

DIABATIC, ADIABATIC, FORCE = 0, 1, 2  # Representation (general.h)


def setup(ln_energy=0.0, mass=2000.0, x0=-8.0, xmin=-15.0, xmax=15.0, dx_max=0.1, dt_max=0.1, number_of_output=50, p0=None, sigma_p=None,
          output_time=None, dx=None, dt=None):
    """The run's constants: input.py's defaults (p0 = sqrt(2 m e^lnE), sigma_p = p0 / 20, output time from the 1-2-5 rounding), then
    main.cpp:41-116.  dx / dt (optional) replace the spacing and step main.cpp:64 and :110 derive (coarse grids for tests and probes)."""
    if p0 is None:
        p0 = float(np.sqrt(2.0 * mass * np.exp(ln_energy)))
    if sigma_p is None:
        sigma_p = p0 / 20.0
    if output_time is None:
        output_time = float(output_time_cutoff((-x0 - x0) / (p0 / mass) / number_of_output))
    sigma_x = HBAR / 2.0 / sigma_p                                           # main.cpp:48
    p0max = p0 + 3.0 * sigma_p                                               # main.cpp:52
    length_x = xmax - xmin                                                   # main.cpp:60
    if dx is None:
        dx = cutoff(min(dx_max, 2.0 * math.pi * HBAR / p0max / 2.0))         # main.cpp:64
    n = int(length_x / dx) + 1                                               # main.cpp:67
    pmin, pmax = p0 - math.pi * HBAR / dx / 2.0, p0 + math.pi * HBAR / dx / 2.0  # main.cpp:70-71
    length_p = pmax - pmin                                                   # main.cpp:72
    dp = length_p / (n - 1)                                                  # main.cpp:73
    i = np.arange(n, dtype=np.float64)
    x = (xmin * (n - 1 - i) + xmax * i) / (n - 1)                            # main.cpp:89
    p = (pmin * (n - 1 - i) + pmax * i) / (n - 1)                            # main.cpp:91
    total_time = length_x / (p0 / mass) * 2.0                                # main.cpp:106
    if dt is None:
        dt = cutoff(min(dt_max, HBAR / 500.0 / (sigma_p * p0 / mass)))       # main.cpp:110
    return dict(mass=mass, x0=x0, p0=p0, sigma_p=sigma_p, sigma_x=sigma_x, xmin=xmin, xmax=xmax, pmin=pmin, pmax=pmax, dx=dx, dp=dp, n_grids=n,
                x=x, p=p, length_x=length_x, length_p=length_p, total_time=total_time, output_time=output_time, dt=dt,
                total_step=int(total_time / dt), output_step=int(output_time / dt))  # main.cpp:114-115


def initial_density(x, p, dx, dp, x0, p0, sigma_x, sigma_p, num_pes):
    """general.cpp:68-106: rho_00 = exp(-((x - x0) / sigma_x)^2 / 2 - ((p - p0) / sigma_p)^2 / 2) / (2 pi sigma_x sigma_p) divided by its grid
    sum times dx dp; every other element zero.  Adiabatic basis.  -> (num_pes, num_pes, n, n) complex"""
    g = np.exp(-(((x[:, None] - x0) / sigma_x) ** 2 + ((p[None, :] - p0) / sigma_p) ** 2) / 2.0) / (2.0 * math.pi * sigma_x * sigma_p)
    rho = np.zeros((num_pes, num_pes, len(x), len(p)), dtype=np.complex128)
    rho[0, 0] = g / (g.sum() * dx * dp)
    return rho


def host_observe(rho_adia, energies, x, p, mass, dx, dp):
    """calculate_average / calculate_population (general.cpp:108-164) of an adiabatic rho on the host (the t = 0 output, main.cpp:155-183)"""
    num_pes = rho_adia.shape[0]
    ppl = np.stack([rho_adia[a, a].real for a in range(num_pes)])
    E = sum((ppl[a] * (energies[:, a][:, None] + p[None, :] ** 2 / 2.0 / mass)).sum() for a in range(num_pes)) * dx * dp
    X = (ppl.sum(axis=0) * x[:, None]).sum() * dx * dp
    P = (ppl.sum(axis=0) * p[None, :]).sum() * dx * dp
    return np.array([E, X, P]), ppl.sum(axis=(1, 2)) * dx * dp


def populations(rho, dx, dp):
    """calculate_population of whatever basis rho is in (general.cpp:108-130)"""
    return np.array([rho[a, a].real.sum() for a in range(rho.shape[0])]) * dx * dp


def averages_line(t, av, pops):
    """One line of averages.txt (main.cpp:170-183, 286-299): t <E> <x> <p> populations"""
    return " ".join(fmt(v) for v in [t, *av, *pops]) + "\n"


def final_line(model, p0, mass, pops):
    """main.cpp:321-335: log(p0^2 / 2m) for DAC, else p0, then the populations of the state as left"""
    head = math.log(p0 * p0 / 2.0 / mass) if model == DAC else p0
    return " ".join(fmt(v) for v in [head, *pops])


def stop_criterion(x_bar, last_x, p0, x0):
    """main.cpp:302 (no population-stable clause)"""
    return x_bar > 0 and ((x_bar - last_x) * p0 < 0 or x_bar > -x0)


def run(api, model=DAC, num_pes=2, ln_energy=0.0, out_dir=None, write_phase="text", max_outputs=None, log=None, on_output=None, **setup_kw):
    """The loop of main.cpp:117-337.  write_phase: "text" (phase.txt), "npy" (phase_<k>.npy per output time) or None; out_dir None writes no
    file.  max_outputs caps the output times after t = 0.  on_output(t, rho_adia) (optional) is called at every output time, t = 0 included, with
    the adiabatic state that phase.txt holds (reconstruct.run_mqcl hangs the GP reconstruction on it).  Returns a dict with the setup,
    per-output records, the final state and the final line."""
    s = setup(ln_energy, **setup_kw)
    n, x, p, mass, dx, dp = s["n_grids"], s["x"], s["p"], s["mass"], s["dx"], s["dp"]
    say = log or (lambda *_: None)
    say(f"dx = {dx:g}, dp = {dp:g}, {n} grids; dt = {s['dt']:g}, {s['total_step']} steps, output every {s['output_step']}")
    t0 = time.perf_counter()
    energies = api.pes_adiabatic_n(num_pes, model, x)[0]
    rho = initial_density(x, p, dx, dp, s["x0"], s["p0"], s["sigma_x"], s["sigma_p"], num_pes)
    files = {}
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        write_grid(os.path.join(out_dir, "x.txt"), x)
        write_grid(os.path.join(out_dir, "p.txt"), p)
        for name in ("t.txt", "averages.txt"):
            files[name] = open(os.path.join(out_dir, name), "w")
        if write_phase == "text":
            files["phase.txt"] = open(os.path.join(out_dir, "phase.txt"), "wb")
    device_text = hasattr(api, "format_g")  # phase.txt converted on the device; an api without it keeps the Python writer
    records = []

    def emit(t, adia, av, pops):
        records.append(dict(t=t, E=av[0], x=av[1], p=av[2], populations=pops))
        if out_dir is None:
            return
        files["t.txt"].write(fmt(t) + "\n")
        files["averages.txt"].write(averages_line(t, av, pops))
        if write_phase == "text":
            files["phase.txt"].write(phase_text(api, adia[None]) if device_text else phase_block(adia).encode())
        elif write_phase == "npy":
            np.save(os.path.join(out_dir, f"phase_{len(records) - 1}.npy"), adia)

    def emit_and_tell(t, adia, av, pops):
        emit(t, adia, av, pops)
        if on_output is not None:
            on_output(t, adia)

    stopped = False
    try:
        av, pops = host_observe(rho, energies, x, p, mass, dx, dp)
        emit_and_tell(0.0, rho, av, pops)
        last_x = av[1]
        rho = api.mqcl_transform(num_pes, model, x, rho, ADIABATIC, DIABATIC)       # main.cpp:185
        n_out = s["total_step"] // s["output_step"]
        if max_outputs is not None:
            n_out = min(n_out, max_outputs)
        t_loop = time.perf_counter()
        for k in range(1, n_out + 1):
            rho = api.mqcl_evolve(num_pes, model, x, p, rho, mass, s["length_x"], s["length_p"], s["dt"], s["output_step"])
            t = k * s["output_step"] * s["dt"]                                        # main.cpp:265
            adia, av, pops = api.mqcl_observe(num_pes, model, x, p, rho, mass, dx, dp)
            emit_and_tell(t, adia, av, pops)
            if stop_criterion(av[1], last_x, s["p0"], s["x0"]):
                stopped = True
                rho = adia                                                            # the loop breaks with rho adiabatic (main.cpp:266, 305)
                break
            last_x = av[1]
    finally:
        for f in files.values():
            f.close()
    t_end = time.perf_counter()
    final_pops = populations(rho, dx, dp)
    line = final_line(model, s["p0"], mass, final_pops)
    say("STOPPED" if stopped else "FINISHED ALL OUTPUT TIMES")
    return dict(setup=s, records=records, stopped=stopped, final_line=line, final_basis=ADIABATIC if stopped else DIABATIC, rho=rho,
                total_seconds=t_end - t0, seconds_per_output=(t_end - t_loop) / max(1, len(records) - 1))
