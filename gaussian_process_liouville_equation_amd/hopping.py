"""Fewest-switches surface hopping (Tully, J. Chem. Phys. 93, 1061 (1990)) on the library's device entry points gple_hop_sample, gple_hop_evolve
and gple_hop_observe: the trajectory baseline of the same model, energy and packet the exact solvers of exact.py and exact_mqcl.py
run.  The reference has no trajectory code; the run's constants are those of exact.setup(boundary=ABSORBING), so its scattering line lines up
column for column with exact.run(flux=True)'s.

    unpack()   the sums of gple_hop_observe as counts, populations and means
    run()      sample, then per output time one hop_evolve of output_step steps and one hop_observe; t.txt and averages.txt
"""
import os
import time

import numpy as np

from . import exact

SAC, DAC, ECR, TSAC = exact.SAC, exact.DAC, exact.ECR, exact.TSAC
RUNNING, LEFT, RIGHT = 0, 1, 2  # the status of a trajectory


def unpack(sums, num_pes, n_traj):
    """The 4 num_pes + 3 sums of hop_observe over n_traj trajectories -> counts (3, num_pes) [status][surface], populations (num_pes,) = mean |c_k|^2,
    x, p, E = the means of x, p and p^2 / 2m + E_surface"""
    sums = np.asarray(sums, dtype=np.float64)
    if sums.shape != (4 * num_pes + 3,):
        raise ValueError("hop_observe returns 4 num_pes + 3 sums")
    return dict(counts=sums[:3 * num_pes].reshape(3, num_pes).copy(), populations=sums[3 * num_pes:4 * num_pes] / n_traj, x=sums[4 * num_pes] / n_traj,
                p=sums[4 * num_pes + 1] / n_traj, E=sums[4 * num_pes + 2] / n_traj)


def averages_line(t, rec, n_traj):
    """One line of averages.txt: t <E> <x> <p>, the fraction of trajectories on each active surface, the mean |c_k|^2 per adiabatic state"""
    return " ".join(exact.fmt(v) for v in [t, rec["E"], rec["x"], rec["p"], *(rec["counts"].sum(axis=0) / n_traj), *rec["populations"]]) + "\n"


def run(api, model=DAC, num_pes=2, ln_energy=0.0, n_traj=10000, seed=0, out_dir=None, reverse_frustrated=False, dt=None, surface0=0, max_outputs=None,
        log=None, **setup_kw):
    """n_traj trajectories from the packet of exact.setup(ln_energy, boundary=ABSORBING, **setup_kw) (x0, sigma_x, p0, sigma_p, mass) on the adiabatic
    surface surface0, evolved with the time step dt (default: the setup's dt_rule, the reference's own rule) between x_left = xmin and
    x_right = xmax; a trajectory that leaves is finished and counted by side and active surface.  The ensemble stays on the device: every
    output time costs one hop_evolve of output_step = int(output_time / dt) steps and one hop_observe, whose 4 num_pes + 3 sums are all that
    crosses.  The run stops when no trajectory is running, or at total_time.  out_dir: t.txt (a time per line) and averages.txt (averages_line);
    None writes no file.  reverse_frustrated: GPLE_HOP_REVERSE.  max_outputs caps the output times (the one at t = 0 included).
    Returns the setup, the records (t and unpack() per output time), stop, and scattering_line: the head of exact.run's final line, the
    fractions that left [left | right][surface], and the fraction still running."""
    setup_kw["boundary"] = exact.ABSORBING
    s = exact.setup(ln_energy, **setup_kw)
    num_pes, n_traj = int(num_pes), int(n_traj)
    dt = float(s["dt_rule"] if dt is None else dt)
    output_step, total_step = int(s["output_time"] / dt), int(s["total_time"] / dt)
    if output_step < 1:
        raise ValueError("the output time is shorter than one time step")
    say = log or (lambda *_: None)
    t0 = time.perf_counter()
    state = api.hop_sample(num_pes, model, n_traj, seed, s["x0"], s["p0"], s["sigma_x"], s["sigma_p"], surface0, device_out=True)
    files = {}
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        files = {name: open(os.path.join(out_dir, name), "w") for name in ("t.txt", "averages.txt")}
    records, stop, step = [], None, 0
    try:
        while True:
            rec = unpack(api.hop_observe(num_pes, model, state, s["mass"]), num_pes, n_traj)
            rec["t"] = step * dt
            records.append(rec)
            if files:
                files["t.txt"].write(exact.fmt(rec["t"]) + "\n")
                files["averages.txt"].write(averages_line(rec["t"], rec, n_traj))
            if rec["counts"][RUNNING].sum() == 0:
                stop = f"NO TRAJECTORY IS RUNNING, STOP EVOLVING AT {rec['t']:g}"
                break
            if step + output_step > total_step or (max_outputs is not None and len(records) >= max_outputs):
                break
            state = api.hop_evolve(num_pes, model, state, seed, s["mass"], dt, step, output_step, s["xmin"], s["xmax"], reverse=reverse_frustrated)
            step += output_step
    finally:
        for f in files.values():
            f.close()
    t_end = time.perf_counter()
    say(stop or "FINISHED ALL OUTPUT TIMES")
    counts = records[-1]["counts"]
    head = np.log(s["p0"] ** 2 / 2.0 / s["mass"]) if model == DAC else s["p0"]  # as exact.run (main.cpp:308-321)
    scattered = np.concatenate([counts[LEFT], counts[RIGHT]]) / n_traj
    line = " ".join(exact.fmt(v) for v in [head, *scattered, counts[RUNNING].sum() / n_traj])
    return dict(setup=s, dt=dt, output_step=output_step, total_step=total_step, n_traj=n_traj, records=records, stop=stop, state=state,
                scattered=scattered.reshape(2, num_pes), scattering_line=line, stop_time=records[-1]["t"], steps=step, total_seconds=t_end - t0)
