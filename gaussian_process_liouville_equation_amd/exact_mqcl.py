"""Exact MQCLE phase-space dynamics: the reference's liouville_equation/main.cpp restated on the library's device entry points
(gple_mqcl_transform, gple_mqcl_evolve, gple_mqcl_observe).

    setup()            main.cpp:41-116 with the defaults of schrodinger_equation/input.py (liouville_equation/ reads the same input file)
    initial_density()  density_matrix_initialization (general.cpp:68-106): a Gaussian in rho_00 of the adiabatic basis, normalised on the grid
    run()              the output loop of main.cpp:117-337: evolve OutputStep steps, observe, write, the stop criterion of :302, the final line
    writers            x.txt, p.txt, t.txt, phase.txt, averages.txt in the reference's line layout; numbers as %g (exact.py)
    boundary=ABSORBING (not in the reference; DESIGN.md §12, "The absorbing boundary"): setup() adds the absorber's rows, the mask interval and
                       the half-mask g; run() puts every block of steps between two half-masks (gple_mqcl_evolve_absorbing) and ends in the
                       scattering line of exact.run(flux=True): absorbed.txt, absorbed_p.txt
"""
import math
import os
import time

import numpy as np

from .exact import ABSORBING, DAC, HBAR, PERIODIC, PPL_LIM, absorbing_potential, cutoff, fmt, output_time_cutoff, phase_block, phase_text, write_grid

DIABATIC, ADIABATIC, FORCE = 0, 1, 2  # Representation (general.h)


def setup(ln_energy=0.0, mass=2000.0, x0=-8.0, xmin=-15.0, xmax=15.0, dx_max=0.1, dt_max=0.1, number_of_output=50, p0=None, sigma_p=None,
          output_time=None, dx=None, dt=None, boundary=PERIODIC):
    """The run's constants: input.py's defaults (p0 = sqrt(2 m e^lnE), sigma_p = p0 / 20, output time from the 1-2-5 rounding), then
    main.cpp:41-116.  dx / dt (optional) replace the spacing and step main.cpp:64 and :110 derive (coarse grids for tests and probes).
    boundary=ABSORBING ("The absorbing boundary") adds n_absorbing = int(absorbing_length / dx) rows on either side of the box,
    absorbing_length = 2 pi hbar / (p0 - 3 sigma_p) as exact.setup has it: x runs from xmin - n_absorbing dx to xmax + n_absorbing dx by the
    interpolation rule of main.cpp:89 and length_x is their difference; p, dt, the step counts and the output time stay.  mask_every is the
    largest divisor of output_step for which the fastest component crosses at most one spacing between two masks,
    (p0 + 3 sigma_p) / m dt mask_every <= dx (at least 1); n_left the number of rows with x <= xmin; g the half-mask of half_mask()."""
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
    total_time = length_x / (p0 / mass) * 2.0                                # main.cpp:106
    extra, x_first, x_last = {}, xmin, xmax
    if boundary == ABSORBING:
        absorbing_length = 2.0 * math.pi * HBAR / (p0 - 3.0 * sigma_p)
        n_abs = int(absorbing_length / dx)
        n += 2 * n_abs
        x_first, x_last = xmin - n_abs * dx, xmax + n_abs * dx
        length_x = x_last - x_first
        extra = dict(absorbing_length=absorbing_length, n_absorbing=n_abs)
    elif boundary != PERIODIC:
        raise ValueError("boundary is PERIODIC or ABSORBING")
    pmin, pmax = p0 - math.pi * HBAR / dx / 2.0, p0 + math.pi * HBAR / dx / 2.0  # main.cpp:70-71
    length_p = pmax - pmin                                                   # main.cpp:72
    dp = length_p / (n - 1)                                                  # main.cpp:73
    i = np.arange(n, dtype=np.float64)
    x = (x_first * (n - 1 - i) + x_last * i) / (n - 1)                       # main.cpp:89
    p = (pmin * (n - 1 - i) + pmax * i) / (n - 1)                            # main.cpp:91
    if dt is None:
        dt = cutoff(min(dt_max, HBAR / 500.0 / (sigma_p * p0 / mass)))       # main.cpp:110
    if boundary == ABSORBING:
        output_step = int(output_time / dt)
        reach = dx / (p0max / mass * dt)  # the steps in which the fastest component crosses one spacing
        extra["mask_every"] = max([k for k in range(1, output_step + 1) if output_step % k == 0 and k <= reach], default=1)
        extra["n_left"] = int(np.sum(x <= xmin))
        extra["g"] = half_mask(x, mass, xmin, xmax, absorbing_length, extra["mask_every"] * dt)
    return dict(**extra, mass=mass, x0=x0, p0=p0, sigma_p=sigma_p, sigma_x=sigma_x, xmin=xmin, xmax=xmax, pmin=pmin, pmax=pmax, dx=dx, dp=dp, n_grids=n,
                x=x, p=p, length_x=length_x, length_p=length_p, total_time=total_time, output_time=output_time, dt=dt,
                total_step=int(total_time / dt), output_step=int(output_time / dt))  # main.cpp:114-115


def half_mask(x, mass, xmin, xmax, absorbing_length, tau):
    """g_i = 1 - exp(-W(x_i) tau / hbar) of the half-mask around a block of duration tau, W from exact.absorbing_potential:
    exactly 0 where W is, 1 where W is not finite; a W that rounding left a hair below zero at the box's edge counts as 0."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        w = absorbing_potential(x, mass, xmin, xmax, absorbing_length)
        g = -np.expm1(-w * tau / HBAR)
    return np.clip(np.where(np.isfinite(w), g, 1.0), 0.0, 1.0)


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


def absorbed_line(t, absorbed, left):
    """One line of absorbed.txt, the layout of exact.run(flux=True): t, the 2 num_pes figures [left | right][surface], the population left"""
    return " ".join(fmt(v) for v in [t, *np.ravel(absorbed), left]) + "\n"


def _to_host(a):
    return a.cpu().numpy() if hasattr(a, "data_ptr") else np.asarray(a)


def run_absorbing(api, model, num_pes, ln_energy, out_dir, write_phase, max_outputs, log, on_output, until_absorbed, mask_every, setup_kw):
    """run(boundary=ABSORBING): the output loop with the half-masks of DESIGN.md §12 around every block of mask_every steps.  On a device api
    the state and the accumulator [side][surface][j] stay on the device: per output one mqcl_evolve_absorbing and one mqcl_observe; what comes
    back is the averages, the populations and the accumulator."""
    s = setup(ln_energy, boundary=ABSORBING, **setup_kw)
    if s["output_step"] < 1:
        raise ValueError("the output time is shorter than one time step")
    if mask_every is not None:
        if mask_every < 1 or s["output_step"] % mask_every:
            raise ValueError("mask_every divides the steps of an output")
        s["mask_every"] = int(mask_every)
        s["g"] = half_mask(s["x"], s["mass"], s["xmin"], s["xmax"], s["absorbing_length"], mask_every * s["dt"])
    n, x, p, mass, dx, dp, g = s["n_grids"], s["x"], s["p"], s["mass"], s["dx"], s["dp"], s["g"]
    say = log or (lambda *_: None)
    say(f"dx = {dx:g}, dp = {dp:g}, {n} grids from {x[0]:g} to {x[-1]:g} ({s['n_absorbing']} absorbing rows a side); dt = {s['dt']:g}, "
        f"{s['total_step']} steps, output every {s['output_step']}, a mask pair every {s['mask_every']}")
    t0 = time.perf_counter()
    energies = api.pes_adiabatic_n(num_pes, model, x)[0]
    rho = initial_density(x, p, dx, dp, s["x0"], s["p0"], s["sigma_x"], s["sigma_p"], num_pes)
    files = {}
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        write_grid(os.path.join(out_dir, "x.txt"), x)
        write_grid(os.path.join(out_dir, "p.txt"), p)
        for name in ("t.txt", "averages.txt", "absorbed.txt"):
            files[name] = open(os.path.join(out_dir, name), "w")
        if write_phase == "text":
            files["phase.txt"] = open(os.path.join(out_dir, "phase.txt"), "wb")
    device_text = hasattr(api, "format_g")
    records = []

    def emit(t, adia, av, pops, absorbed):
        records.append(dict(t=t, E=av[0], x=av[1], p=av[2], populations=pops, absorbed=absorbed))
        if out_dir is not None:
            files["t.txt"].write(fmt(t) + "\n")
            files["averages.txt"].write(averages_line(t, av, pops))
            files["absorbed.txt"].write(absorbed_line(t, absorbed, float(np.sum(pops))))
            if write_phase == "text":
                files["phase.txt"].write(phase_text(api, adia[None]) if device_text else phase_block(_to_host(adia)).encode())
            elif write_phase == "npy":
                np.save(os.path.join(out_dir, f"phase_{len(records) - 1}.npy"), _to_host(adia))
        if on_output is not None:
            on_output(t, adia)

    stop = None
    acc = np.zeros((2, num_pes, n))
    want_adia = on_output is not None or (out_dir is not None and write_phase is not None)
    try:
        av, pops = host_observe(rho, energies, x, p, mass, dx, dp)
        emit(0.0, rho, av, pops, np.zeros((2, num_pes)))
        last_x = av[1]
        rho = api.mqcl_transform(num_pes, model, x, rho, ADIABATIC, DIABATIC)
        dx_, dp_, dg_ = x, p, g
        if getattr(api, "device", None) is not None:
            import torch
            where = torch.device("cuda", api.device)
            dx_, dp_, dg_, rho, acc = (torch.from_numpy(a).to(where) for a in (x, p, g, rho, acc))
            torch.cuda.synchronize(where)  # the uploads, before the context's stream reads them
        n_out = s["total_step"] // s["output_step"]
        if max_outputs is not None:
            n_out = min(n_out, max_outputs)
        t_loop = time.perf_counter()
        for k in range(1, n_out + 1):
            rho, acc = api.mqcl_evolve_absorbing(num_pes, model, dx_, dp_, rho, mass, s["length_x"], s["length_p"], s["dt"], s["output_step"], s["mask_every"],
                                                 dg_, s["n_left"], acc)
            t = k * s["output_step"] * s["dt"]
            adia, av, pops = api.mqcl_observe(num_pes, model, dx_, dp_, rho, mass, dx, dp, adiabatic=want_adia)
            if hasattr(api, "synchronize"):
                api.synchronize()
            av, pops = _to_host(av), _to_host(pops)
            emit(t, adia, av, pops, _to_host(acc).sum(axis=2) * (dx * dp))
            if float(np.sum(pops)) < PPL_LIM:
                stop = f"ALMOST ALL POPULATION HAVE BEEN ABSORBED, STOP EVOLVING AT {t:g}"
            elif not until_absorbed and stop_criterion(av[1], last_x, s["p0"], s["x0"]):
                stop = f"GET OUT OF INTERACTING REGION OR DIRECTION REVERSED, STOP EVOLVING AT {t:g}"
            if stop:
                break
            last_x = av[1]
        absorbed_p = _to_host(acc) * dx
        if out_dir is not None:
            with open(os.path.join(out_dir, "absorbed_p.txt"), "w") as f:
                f.write("".join(" ".join(fmt(v) for v in row) + "\n" for row in absorbed_p.reshape(2 * num_pes, n)))
    finally:
        for f in files.values():
            f.close()
    t_end = time.perf_counter()
    last = records[-1]
    head = math.log(s["p0"] * s["p0"] / 2.0 / mass) if model == DAC else s["p0"]
    say(stop or "FINISHED ALL OUTPUT TIMES")
    return dict(setup=s, records=records, stopped=stop is not None, stop=stop, final_line=final_line(model, s["p0"], mass, last["populations"]),
                final_basis=DIABATIC, rho=rho, absorbed=last["absorbed"], absorbed_p=absorbed_p, stop_time=last["t"],
                scattering_line=" ".join(fmt(v) for v in [head, *last["absorbed"].ravel(), float(np.sum(last["populations"]))]),
                total_seconds=t_end - t0, seconds_per_output=(t_end - t_loop) / max(1, len(records) - 1))


def run(api, model=DAC, num_pes=2, ln_energy=0.0, out_dir=None, write_phase="text", max_outputs=None, log=None, on_output=None, boundary=PERIODIC,
        until_absorbed=False, mask_every=None, **setup_kw):
    """The loop of main.cpp:117-337.  write_phase: "text" (phase.txt), "npy" (phase_<k>.npy per output time) or None; out_dir None writes no
    file.  max_outputs caps the output times after t = 0.  on_output(t, rho_adia) (optional) is called at every output time, t = 0 included, with
    the adiabatic state that phase.txt holds (reconstruct.run_mqcl hangs the GP reconstruction on it).  Returns a dict with the setup,
    per-output records, the final state and the final line.
    boundary=ABSORBING ("The absorbing boundary"): the box grows by the absorber of setup(boundary=ABSORBING) and every block of
    mask_every steps (None: the set-up's) runs between two half-masks, which book what they remove per side of the box, adiabatic surface and
    momentum index.  Every record carries `absorbed` (2, num_pes), [left | right][surface]: what has left up to its output time; it and the
    populations left add up to the initial population to rounding, and a figure may be slightly negative.  absorbed.txt has exact.run(flux=True)'s
    layout (t, the 2 num_pes figures, the population left); absorbed_p.txt, written at the end, has a line per (side, surface) with the n values
    of the outgoing momentum distribution (the accumulator times dx).  The result gains `absorbed`, `absorbed_p` (2, num_pes, n) and
    `scattering_line`, whose columns are those of exact.run(flux=True)'s and hopping.run's.  The run stops when less than PPL_LIM is left; with
    until_absorbed that is the only stop, otherwise the criterion of main.cpp:302 applies too; otherwise it ends with the output times.  The
    final state is the diabatic one (a device tensor on a device api)."""
    if boundary == ABSORBING:
        return run_absorbing(api, model, num_pes, ln_energy, out_dir, write_phase, max_outputs, log, on_output, until_absorbed, mask_every, setup_kw)
    if boundary != PERIODIC or until_absorbed or mask_every is not None:
        raise ValueError("until_absorbed and mask_every belong to boundary=ABSORBING")
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
