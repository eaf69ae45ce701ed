"""Fewest-switches surface hopping (Tully, J. Chem. Phys. 93, 1061 (1990)) on the library's device entry points gple_hop_sample, gple_hop_evolve
and gple_hop_observe: the trajectory baseline of the same model, energy and packet the exact solvers of exact.py and exact_mqcl.py
run.  The reference has no trajectory code; the run's constants are those of exact.setup(boundary=ABSORBING), so its scattering line lines up
column for column with exact.run(flux=True)'s.

    unpack()          the sums of gple_hop_observe as counts, populations and means
    phase_grid_of()   the phase-space grid of a run, from its size
    run()             sample, then per output time one hop_evolve of output_step steps and one hop_observe; t.txt and averages.txt.  With a
                      phase_grid also one gple_hop_bin and gple_hop_density: x.txt, p.txt and phase.txt, the adiabatic density of the ensemble
                      (phase_density="amplitude": gple_hop_bin_mf and gple_hop_density_mf, which "ehrenfest" runs have too).  With phase_smooth
                      the phase.txt block is the Gaussian kernel density estimate of gple_hop_smooth (_mf) instead.  With outgoing
                      also one gple_hop_outgoing (_mf, _sqc) per axis on the final state: outgoing_p.txt and outgoing_e.txt, what left the
                      box per side and level by momentum and by energy (outgoing_density(), outgoing_grids(), write_outgoing())
    scan()            the branching probabilities at many momenta from one grouped ensemble (gple_hop_sample_groups / _evolve_groups /
                      _observe_groups): a group per momentum with its own packet and time step; scan.txt
run() and scan() take decoherence = None (Tully's algorithm as it stands), "edc", "collapse_hop" or "collapse_attempt" and edc_c: the decoherence
correction of every step (gple_hop_evolve_dc / gple_hop_evolve_groups_dc; DESIGN.md §17, "Decoherence corrections").  The files are the same.
run() and scan() are one loop each, written against the record of their method in TABLE (a Method: which api calls sample, evolve and observe,
how the arguments of the step are built, how its sums are read, what it refuses):
    "fssh"       the default, everything above
    "ehrenfest"  mean-field trajectories from the same sample: hop_evolve_mf / hop_observe_mf, unpack_mf(); no hops, nothing random
    "sqc"        the Meyer-Miller-Stock-Thoss mapping Hamiltonian with the windows of Cotton and Miller: window = "triangle" (the default) or
                 "square" and gamma (None: 1 / 3 or (sqrt(3) - 1) / 2); hop_sample_sqc / hop_evolve_sqc / hop_observe_sqc, unpack_sqc()
    "mash"       the mapping approach to surface hopping of Mannouch and Richardson, two levels only: hop_sample_mash / hop_evolve_mash, then
                 the sums, the records and every file of "fssh"
each with its _groups forms in scan() (DESIGN.md §17 has a section per method).  A new method is one more record.
"""
import os
import time
from typing import Callable, NamedTuple, Optional

import numpy as np

from . import exact
from ._capi import HOP_WINDOW_GAMMA, HOP_WINDOW_NAMES, HOP_WINDOW_SQUARE

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


METHODS = ("fssh", "ehrenfest")


def unpack_mf(sums, num_pes, n_traj):
    """The 3 num_pes + 6 sums of hop_observe_mf over n_traj trajectories -> weights (3, num_pes) [status][k] = sum |c_k|^2 over the trajectories of
    that status, n_status (3,) the trajectories per status, populations (num_pes,) = mean |c_k|^2 over all of them, x, p, E = the means of x, p
    and p^2 / 2m + sum_k |c_k|^2 E_k; counts = weights, so that the scattering line is built by the code that builds it from unpack()"""
    sums = np.asarray(sums, dtype=np.float64)
    if sums.shape != (3 * num_pes + 6,):
        raise ValueError("hop_observe_mf returns 3 num_pes + 6 sums")
    weights = sums[:3 * num_pes].reshape(3, num_pes).copy()
    return dict(weights=weights, counts=weights, n_status=sums[3 * num_pes:3 * num_pes + 3].copy(), populations=weights.sum(axis=0) / n_traj,
                x=sums[3 * num_pes + 3] / n_traj, p=sums[3 * num_pes + 4] / n_traj, E=sums[3 * num_pes + 5] / n_traj)


def averages_line_mf(t, rec):
    """One line of a mean-field averages.txt: t <E> <x> <p>, the mean |c_k|^2 per adiabatic state (there is no active surface to count)"""
    return " ".join(exact.fmt(v) for v in [t, rec["E"], rec["x"], rec["p"], *rec["populations"]]) + "\n"


SQC = "sqc"  # the third method: its ensemble comes from a sample of its own (hop_sample_sqc), METHODS are the two that share hop_sample's


MASH = "mash"  # the fourth method: a sample and a step of its own, the sums of "fssh"


PHASE_DENSITIES = (None, "mixed", "amplitude")  # run(phase_density=...): None is "mixed"


def sqc_window(window, gamma):
    """(GPLE_HOP_WINDOW_*, gamma) of run() and scan(): window "triangle" (None) or "square"; gamma None is the window's customary value, 1 / 3 or
    (sqrt(3) - 1) / 2.  What the library would refuse is a ValueError here, before any call"""
    name = "triangle" if window is None else window
    if name not in HOP_WINDOW_NAMES:
        raise ValueError(f"window is one of {sorted(HOP_WINDOW_NAMES)}")
    code = HOP_WINDOW_NAMES[name]
    gamma = HOP_WINDOW_GAMMA[code] if gamma is None else float(gamma)
    if not np.isfinite(gamma) or gamma < 0.0 or (code == HOP_WINDOW_SQUARE and not 0.0 < gamma < 0.5):
        raise ValueError("gamma is finite and not negative, and inside (0, 1/2) for the square window")
    return code, gamma


def unpack_sqc(sums, num_pes, n_traj, gamma):
    """The 4 num_pes + 9 sums of hop_observe_sqc over n_traj trajectories -> counts (3, num_pes) [status][k] the trajectories of that status in
    the window of state k, n_status (3,) the trajectories per status, none (3,) those of each status in no window (counts.sum(1) + none ==
    n_status), e (num_pes,) = mean e_k, actions = e - gamma, windowed (num_pes,) the fraction of ALL trajectories in window k, unassigned the
    fraction in none, x, p, E = the means of x, p and H = p^2 / 2m + sum_k (e_k - gamma) E_k"""
    sums = np.asarray(sums, dtype=np.float64)
    N = num_pes
    if sums.shape != (4 * N + 9,):
        raise ValueError("hop_observe_sqc returns 4 num_pes + 9 sums")
    counts = sums[:3 * N].reshape(3, N).copy()
    e = sums[3 * N + 6:4 * N + 6] / n_traj
    return dict(counts=counts, n_status=sums[3 * N:3 * N + 3].copy(), none=sums[3 * N + 3:3 * N + 6].copy(), e=e, actions=e - gamma,
                windowed=counts.sum(axis=0) / n_traj, unassigned=sums[3 * N + 3:3 * N + 6].sum() / n_traj, x=sums[4 * N + 6] / n_traj,
                p=sums[4 * N + 7] / n_traj, E=sums[4 * N + 8] / n_traj)


def averages_line_sqc(t, rec):
    """One line of an SQC averages.txt: t <E> <x> <p>, the windowed fraction per state over all statuses, the mean action per state, the
    unassigned fraction"""
    return " ".join(exact.fmt(v) for v in [t, rec["E"], rec["x"], rec["p"], *rec["windowed"], *rec["actions"], rec["unassigned"]]) + "\n"


def sqc_channels(counts, n_status, none):
    """From the last sums of an ensemble (or, with a leading axis, of every group): the channels (..., 2, num_pes) = counts[side][k] / N_f, N_f
    the FINISHED AND WINDOWED trajectories (0 where N_f = 0), N_f itself, and the unassigned fraction of the finished ones (0 where none finished)"""
    counts, n_status, none = (np.asarray(a, dtype=np.float64) for a in (counts, n_status, none))
    finished = counts[..., 1:, :]
    n_f = finished.sum(axis=(-2, -1))
    n_done = n_status[..., 1:].sum(axis=-1)
    channels = np.divide(finished, n_f[..., None, None], out=np.zeros_like(finished), where=n_f[..., None, None] > 0)
    lost = np.divide(none[..., 1:].sum(axis=-1), n_done, out=np.zeros_like(n_done), where=n_done > 0)
    return channels, n_f, lost


# ---- the methods: one record each, which run() and scan() are written against ---------------------------------------------------------------------
# tail below is what a windowed method's calls take beside the others' arguments: sqc_window()'s (code, gamma), else ()
def _seeded_step(seed, reverse, correction, tail, mass, dt, first_step, n_steps, x_left, x_right):
    return (seed, mass, dt, first_step, n_steps, x_left, x_right), dict(reverse=reverse, **correction)


def _plain_step(seed, reverse, correction, tail, mass, dt, first_step, n_steps, x_left, x_right):
    return (mass, dt, n_steps, x_left, x_right, *tail[1:]), {}  # windowed: gamma last


def _on_surface(sums, num_pes):
    return sums[..., :num_pes].sum(axis=-1)


def _of_status(sums, num_pes):
    return sums[..., 3 * num_pes]


def _counted(sums, num_pes, n):
    """counts[side][surface] / n (with "ehrenfest" the weights): every trajectory is in the sample"""
    counts = sums[..., :3 * num_pes].reshape(*sums.shape[:-1], 3, num_pes)
    return counts[..., 1:, :] / n, np.full(sums.shape[:-1], float(n)), ()


def _windowed(sums, num_pes, n):
    """sqc_channels over the finished and windowed trajectories, and as a new last column the unassigned fraction of the finished ones"""
    N = num_pes
    channels, n_f, lost = sqc_channels(sums[..., :3 * N].reshape(*sums.shape[:-1], 3, N), sums[..., 3 * N:3 * N + 3], sums[..., 3 * N + 3:3 * N + 6])
    return channels, n_f, (lost,)


def _sqc_result(result, tail, n_f, last):
    """no correction to report and no phase_density; the window's code, gamma and what sqc_channels counted (numbers from run(), rows from scan())"""
    own = (float(n_f), float(last[0])) if np.ndim(n_f) == 0 else (n_f, last[0])
    result = {key: value for key, value in result.items() if key != "phase_density"}
    return dict(result, decoherence=None, edc_c=None, window=tail[0], gamma=tail[1], n_finished_windowed=own[0], unassigned_finished=own[1])


class Method(NamedTuple):
    """A trajectory method as run() and scan() see it; the defaults are the sums, records and files of "fssh".  sample, evolve, observe: the
    suffix of the api attribute, hop_<verb><suffix> in run() and hop_<verb>_groups<suffix> in scan(), looked up on the api when it is called"""
    sample: str = ""
    evolve: str = ""
    observe: str = ""
    step_args: Callable = _plain_step  # (seed, reverse, correction, tail, mass, dt, first_step, n_steps, x_left, x_right) -> after the ensemble [and n_per_group]; keywords
    width: Callable = lambda num_pes: 4 * num_pes + 3  # the numbers in a row of sums
    unpack: Callable = unpack          # unpack, unpack_mf or unpack_sqc (which takes gamma too)
    line: Callable = averages_line     # (t, rec, n_traj) -> the line of averages.txt
    running: Callable = _on_surface    # (sums (..., width), num_pes) -> the trajectories still running (...)
    channels: Callable = _counted      # (sums (..., width), num_pes, n) -> scattered (..., 2, num_pes), the size (...) of the sample behind it, further last columns
    result: Callable = lambda result, tail, n_f, last: result  # the result all methods share -> the method's
    counters: bool = False             # the grouped step keeps the (n, 2) counters of hops taken and frustrated
    windowed: bool = False             # takes window and gamma
    refusal: Optional[str] = None      # the ValueError of a decoherence correction, reverse_frustrated=True or a phase_grid; None: takes them
    amplitude_grid: bool = False       # takes a phase_grid with phase_density="amplitude" all the same
    two_level: bool = False


_NO_SURFACE = "{} trajectories have no active surface: no decoherence correction, no frustrated hops and (DESIGN.md §17) no phase_grid"
TABLE = {
    "fssh": Method(step_args=_seeded_step, counters=True),
    "ehrenfest": Method(evolve="_mf", observe="_mf", width=lambda num_pes: 3 * num_pes + 6, unpack=unpack_mf, line=lambda t, rec, n_traj: averages_line_mf(t, rec),
                        running=_of_status, refusal=_NO_SURFACE.format("ehrenfest") + ' but with phase_density="amplitude"', amplitude_grid=True),
    SQC: Method(sample="_sqc", evolve="_sqc", observe="_sqc", width=lambda num_pes: 4 * num_pes + 9, unpack=unpack_sqc,
                line=lambda t, rec, n_traj: averages_line_sqc(t, rec), running=_of_status, channels=_windowed, result=_sqc_result, windowed=True,
                refusal=_NO_SURFACE.format(SQC)),
    MASH: Method(sample="_mash", evolve="_mash", counters=True, two_level=True,
                 refusal="mash trajectories need no decoherence correction, always reflect a frustrated hop and (DESIGN.md §17) have no phase_grid"),
}


def _method(method, decoherence, reverse_frustrated, phase_grid=None, window=None, gamma=None, num_pes=2, phase_density=None):
    """method of run() and scan(), checked against the options it refuses -> its record.  phase_density: the prescription of run()'s phase_grid;
    "amplitude" needs no active surface, so "ehrenfest" may have a phase_grid with it (and with it alone)"""
    if method not in TABLE:
        raise ValueError(f"method is one of {tuple(TABLE)}")
    if phase_density not in PHASE_DENSITIES:
        raise ValueError('phase_density is None, "mixed" or "amplitude"')
    if phase_density is not None and phase_grid is None:
        raise ValueError("phase_density belongs to a phase_grid")
    m = TABLE[method]
    if not m.windowed and (window is not None or gamma is not None):
        raise ValueError('window and gamma belong to method="sqc"')
    if m.amplitude_grid and phase_density == "amplitude":
        phase_grid = None  # the density from the amplitudes needs no active surface
    if m.refusal is not None and (decoherence is not None or reverse_frustrated or phase_grid is not None):
        raise ValueError(m.refusal)
    if m.two_level and int(num_pes) != 2:
        raise ValueError(f"{method} is a two-level method: num_pes = 2")
    return m


def _call(api, verb, suffix, grouped=False):
    """the api's hop_<verb>[_groups]<suffix>, looked up now: an api needs the calls of the methods it is asked for, and no others"""
    return getattr(api, f"hop_{verb}{'_groups' if grouped else ''}{suffix}")


def _head(model, s):
    """the first column of a scattering line, as exact.run (main.cpp:308-321): ln E for DAC, else p0"""
    return np.log(s["p0"] ** 2 / 2.0 / s["mass"]) if model == DAC else s["p0"]


GRID_KEYS = ("x_first", "dx", "n_x", "p_first", "dp", "n_p")


def phase_grid_of(api, num_pes, model, s, phase_grid):
    """The grid (x_first, dx, n_x, p_first, dp, n_p) of hop_bin for the setup s.  (n_x, n_p): x_i = xmin + i dx over [xmin, xmax] and p_j over
    [-p_max, p_max] with p_max = sqrt((p0 + 6 sigma_p)^2 + 2 m (E_max - E_min)), E the adiabatic energies on that x grid: a bound, since a
    trajectory conserves p^2 / 2m + E_a and the sample's |p| exceeds p0 + 6 sigma_p with probability below 1e-8.  A dict gives n_x and n_p and
    overrides any of the other four numbers."""
    given = dict(phase_grid) if isinstance(phase_grid, dict) else dict(zip(("n_x", "n_p"), phase_grid))
    if set(given) - set(GRID_KEYS) or "n_x" not in given or "n_p" not in given:
        raise ValueError("phase_grid is (n_x, n_p), or a dict with n_x, n_p and any of x_first, dx, p_first, dp")
    n_x, n_p = int(given["n_x"]), int(given["n_p"])
    if n_x < 1 or n_p < 1 or (n_x < 2 and "dx" not in given) or (n_p < 2 and "dp" not in given):
        raise ValueError("an axis of one point needs its spacing")
    x_first = float(given.get("x_first", s["xmin"]))
    dx = float(given["dx"]) if "dx" in given else (s["xmax"] - s["xmin"]) / (n_x - 1)
    if "p_first" in given and "dp" in given:
        p_first, dp = float(given["p_first"]), float(given["dp"])
    else:
        E = np.asarray(api.pes_adiabatic_n(num_pes, model, x_first + dx * np.arange(n_x))[0], dtype=np.float64)
        p_max = float(np.sqrt((abs(s["p0"]) + 6.0 * s["sigma_p"]) ** 2 + 2.0 * s["mass"] * (E.max() - E.min())))
        p_first = float(given.get("p_first", -p_max))
        dp = float(given["dp"]) if "dp" in given else (p_max - p_first) / (n_p - 1)
    return (x_first, dx, n_x, p_first, dp, n_p)


OUTGOING_AXES = ("momentum", "energy")  # run(outgoing=...): the keys, in the order of their calls


def outgoing_density(acc, num_pes, n_bins, n_norm, step):
    """The accumulator of hop_outgoing (numpy, or a tensor on the GPU, of which only its numbers cross) -> the density (2, num_pes, n_bins)
    float64 [side][level][bin] = (double)sum 2^-32 / (n_norm step), left to right, per unit of the axis and normalised to the n_norm trajectories
    behind the method's scattering line, and the four tallies [binned, outside, running, unassigned] as Python integers"""
    acc = np.asarray(acc.cpu().numpy() if hasattr(acc, "is_cuda") else acc, dtype=np.int64)
    num_pes, n_bins = int(num_pes), int(n_bins)
    if acc.shape != (2 * num_pes * n_bins + 4,):
        raise ValueError("hop_outgoing returns 2 num_pes n_bins + 4 integers")
    w = np.float64(n_norm) * np.float64(step)
    if not w > 0.0:
        raise ValueError("n_norm and step are positive")
    return acc[:-4].reshape(2, num_pes, n_bins).astype(np.float64) * (1.0 / 4294967296.0) / w, tuple(int(v) for v in acc[-4:])


def _outgoing_request(outgoing):
    """run(outgoing=...) checked before any api call -> {axis: a number of bins >= 2, or the triple (first, step, n_bins)} in OUTGOING_AXES' order"""
    if outgoing is None:
        return {}
    if not isinstance(outgoing, dict) or not outgoing or set(outgoing) - set(OUTGOING_AXES):
        raise ValueError(f"outgoing is a dict with any of the keys {OUTGOING_AXES}")
    request = {}
    for axis in OUTGOING_AXES:
        if axis not in outgoing:
            continue
        given = outgoing[axis]
        if isinstance(given, (tuple, list)) and len(given) == 3:
            first, step, n_bins = float(given[0]), float(given[1]), given[2]
            if n_bins != int(n_bins) or int(n_bins) < 1 or not np.isfinite(first) or not np.isfinite(step) or step <= 0.0:
                raise ValueError("an outgoing grid is (first, step, n_bins): first finite, step finite and positive, n_bins >= 1")
            request[axis] = (first, step, int(n_bins))
        elif isinstance(given, (int, np.integer)) and not isinstance(given, bool) and given >= 2:
            request[axis] = int(given)
        else:
            raise ValueError("an outgoing axis is a number of bins (at least 2) or the triple (first, step, n_bins)")
    return request


def outgoing_grids(api, num_pes, model, s, surface0, request):
    """The grids (first, step, n_bins) of run(outgoing=...) for the setup s; a triple is taken as it is.  A number of bins: for the momentum the
    p axis of phase_grid_of(api, num_pes, model, s, (257, n_bins)), which bounds every outgoing momentum; for the energy n_bins points from
    (p0 - 3 sigma_p)^2 / 2m + E0 to (p0 + 3 sigma_p)^2 / 2m + E0, E0 the adiabatic energy of surface0 at x0 (the lower momentum taken as 0
    where it would be negative): a trajectory keeps the energy it was drawn with"""
    grids = {}
    for axis, given in request.items():
        if isinstance(given, tuple):
            grids[axis] = given
        elif axis == OUTGOING_AXES[0]:
            grids[axis] = phase_grid_of(api, num_pes, model, s, (257, given))[3:]
        else:
            E0 = float(np.asarray(api.pes_adiabatic_n(num_pes, model, np.array([s["x0"]]))[0], dtype=np.float64).reshape(-1, num_pes)[0, surface0])
            low, high = (max(p, 0.0) ** 2 / 2.0 / s["mass"] + E0 for p in (s["p0"] - 3.0 * s["sigma_p"], s["p0"] + 3.0 * s["sigma_p"]))
            grids[axis] = (low, (high - low) / (given - 1), given)
    return grids


def _smooth_request(phase_smooth, phase_grid):
    """run(phase_smooth=...) checked before any api call -> None, "scott" or the pair (h_x, h_p) as floats"""
    if phase_smooth is None:
        return None
    if phase_grid is None:
        raise ValueError("phase_smooth belongs to a phase_grid")
    if isinstance(phase_smooth, str):
        if phase_smooth != "scott":
            raise ValueError('phase_smooth is None, "scott" or a pair (h_x, h_p) of finite positive numbers')
        return phase_smooth
    try:
        h_x, h_p = (float(h) for h in phase_smooth)
    except (TypeError, ValueError):
        raise ValueError('phase_smooth is None, "scott" or a pair (h_x, h_p) of finite positive numbers') from None
    if not (np.isfinite(h_x) and np.isfinite(h_p) and h_x > 0.0 and h_p > 0.0):
        raise ValueError('phase_smooth is None, "scott" or a pair (h_x, h_p) of finite positive numbers')
    return (h_x, h_p)


def smooth_bandwidth(request, s, n_traj):
    """The bandwidths (h_x, h_p) of run(phase_smooth=...): a pair as it is; "scott": Scott's rule for a Gaussian kernel in two dimensions,
    h = sigma n_traj^(-1/6) per axis with the packet's sigma_x and sigma_p"""
    if request == "scott":
        factor = float(n_traj) ** (-1.0 / 6.0)
        return (float(s["sigma_x"]) * factor, float(s["sigma_p"]) * factor)
    return request


def write_outgoing(out_dir, axis, grid, density):
    """outgoing_p.txt: a line per (side, level) with the n_bins densities per unit momentum, the layout of exact_mqcl's absorbed_p.txt;
    outgoing_e.txt: a line per bin with E and the 2 num_pes densities per unit energy, the layout of exact's spectrum.txt"""
    flat = density.reshape(-1, density.shape[-1])
    if axis == OUTGOING_AXES[0]:
        name, rows = "outgoing_p.txt", flat
    else:
        name, rows = "outgoing_e.txt", np.column_stack([grid[0] + grid[1] * np.arange(grid[2]), flat.T])
    with open(os.path.join(out_dir, name), "w") as f:
        f.write("".join(" ".join(exact.fmt(v) for v in row) + "\n" for row in rows))


def run(api, model=DAC, num_pes=2, ln_energy=0.0, n_traj=10000, seed=0, out_dir=None, reverse_frustrated=False, dt=None, surface0=0, max_outputs=None,
        log=None, phase_grid=None, decoherence=None, edc_c=0.1, method="fssh", window=None, gamma=None, phase_density=None, outgoing=None, phase_smooth=None,
        **setup_kw):
    """n_traj trajectories from the packet of exact.setup(ln_energy, boundary=ABSORBING, **setup_kw) (x0, sigma_x, p0, sigma_p, mass) on the adiabatic
    surface surface0, evolved with the time step dt (default: the setup's dt_rule, the reference's own rule) between x_left = xmin and
    x_right = xmax; a trajectory that leaves is finished and counted by side and active surface.  The ensemble stays on the device: every
    output time costs one hop_evolve of output_step = int(output_time / dt) steps and one hop_observe, whose 4 num_pes + 3 sums are all that
    crosses.  The run stops when no trajectory is running, or at total_time.  out_dir: t.txt (a time per line) and averages.txt (averages_line);
    None writes no file.  reverse_frustrated: GPLE_HOP_REVERSE.  max_outputs caps the output times (the one at t = 0 included).
    phase_grid (phase_grid_of; None: nothing below happens): every output time also costs one hop_bin of the running trajectories, whose record
    gains binned, outside and binned_counts (per active surface), and with out_dir one hop_density, appended to phase.txt as exact.run writes
    it (the text made on the device where the api has format_g); x.txt and p.txt are written once.  The directory is then what
    reconstruct.run_files reads.
    phase_density (with a phase_grid only): None or "mixed" is the above, call for call: populations from the active surface, coherences from
    the amplitudes.  "amplitude" takes both from the amplitudes (hop_bin_mf / hop_density_mf; DESIGN.md §17, "The ensemble in phase space,
    from the amplitudes"), which is the density of an "ehrenfest" run and the other prescription of an "fssh" one; the files are the same, and
    a record gains binned, outside and binned_weights, the per-state sums of the weight planes times 2^-32 as floats (no binned_counts).
    decoherence (None, "edc", "collapse_hop", "collapse_attempt") and edc_c: the decoherence correction of every step; with None the api is
    called without these keywords, otherwise both are forwarded to every hop_evolve.  The result carries both.
    method: "fssh" (the default: everything above, call for call) or "ehrenfest", mean-field trajectories from the same sample: per output time
    one hop_evolve_mf and one hop_observe_mf, whose record is unpack_mf()'s; the run stops when n_status[0] == 0.  An averages.txt line is then
    averages_line_mf (no active-surface columns), and the scattering line holds weights[left][k] / n, weights[right][k] / n and n_status[0] / n
    in the same columns.  decoherence, reverse_frustrated=True or a phase_grid without phase_density="amplitude" is a ValueError with "ehrenfest".
    method "sqc" with window ("triangle", the default, or "square") and gamma (None: the window's customary value): hop_sample_sqc, then per output
    time one hop_evolve_sqc and one hop_observe_sqc, whose record is unpack_sqc()'s; averages.txt holds averages_line_sqc.  The scattering line
    keeps its columns with channel (side, k) = counts[side][k] / N_f, N_f the finished and windowed trajectories (all 0 where N_f = 0), then
    n_status[0] / n, and as a new last column the unassigned fraction of the finished trajectories.  The same options are a ValueError with it,
    and so are window or gamma with another method.
    method "mash": everything of "fssh" (records, files, the scattering line) with hop_sample_mash for the sample and one hop_evolve_mash per
    output time, which takes no seed and no step number.  decoherence, reverse_frustrated=True, a phase_grid, window, gamma or num_pes != 2 with
    it is a ValueError.
    outgoing (None: nothing below happens, call for call and key for key): a dict with any of the keys "momentum" and "energy", each a number of
    bins, at least 2 on either axis since the default grids take their step from their two ends (the grid of outgoing_grids), or a triple
    (first, step, n_bins), which may have one bin.  After the loop the final state costs one hop_outgoing<suffix> call per
    axis, the suffix being that of the method's observe call ("What left the box"): what left per side and level, resolved in
    the outgoing momentum or in the energy the method conserves.  The result gains `outgoing`: per axis grid, density (outgoing_density with
    n_norm the sample behind the scattering line, so that density step summed over the bins is `scattered` where nothing is outside), acc and
    tallies; with out_dir also outgoing_p.txt and outgoing_e.txt (write_outgoing).  Anything else in outgoing is a ValueError before any call.
    phase_smooth (with a phase_grid only; None: nothing below happens, call for call and key for key): "scott" (smooth_bandwidth: h = sigma
    n_traj^(-1/6) per axis) or a pair (h_x, h_p) of finite positive numbers.  Every output time still makes its hop_bin (or hop_bin_mf) call,
    so binned, outside and binned_counts or binned_weights stay as they are, and also one hop_smooth (phase_density None or "mixed") or
    hop_smooth_mf ("amplitude"), the Gaussian kernel density estimate of DESIGN.md §17, "The ensemble in phase space, smoothed": its field is
    the phase.txt block in place of hop_density's, and the record gains smoothed and nonfinite, the call's two tallies.  The result gains
    phase_smooth, the pair used.  Anything else in phase_smooth, or one without a phase_grid, is a ValueError before any call; a method that
    refuses a phase_grid refuses this with it.
    Returns the setup, the records (t and unpack() per output time), stop, and scattering_line: the head of exact.run's final line, the
    fractions that left [left | right][surface], and the fraction still running."""
    m = _method(method, decoherence, reverse_frustrated, phase_grid, window, gamma, num_pes, phase_density)
    tail = sqc_window(window, gamma) if m.windowed else ()  # what follows surface0 in the sample and mass in the observe
    request = _outgoing_request(outgoing)
    smooth = _smooth_request(phase_smooth, phase_grid)
    amplitude = phase_density == "amplitude"
    setup_kw["boundary"] = exact.ABSORBING
    s = exact.setup(ln_energy, **setup_kw)
    num_pes, n_traj = int(num_pes), int(n_traj)
    dt = float(s["dt_rule"] if dt is None else dt)
    output_step, total_step = int(s["output_time"] / dt), int(s["total_time"] / dt)
    if output_step < 1:
        raise ValueError("the output time is shorter than one time step")
    correction = {} if decoherence is None else dict(decoherence=decoherence, edc_c=edc_c)
    say = log or (lambda *_: None)
    t0 = time.perf_counter()
    state = _call(api, "sample", m.sample)(num_pes, model, n_traj, seed, s["x0"], s["p0"], s["sigma_x"], s["sigma_p"], surface0, *tail, device_out=True)
    grid = None if phase_grid is None else phase_grid_of(api, num_pes, model, s, phase_grid)
    bandwidth = smooth_bandwidth(smooth, s, n_traj)
    files = {}
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        files = {name: open(os.path.join(out_dir, name), "w") for name in ("t.txt", "averages.txt")}
        if grid is not None:
            exact.write_grid(os.path.join(out_dir, "x.txt"), grid[0] + grid[1] * np.arange(grid[2]))
            exact.write_grid(os.path.join(out_dir, "p.txt"), grid[3] + grid[4] * np.arange(grid[5]))
            files["phase.txt"] = open(os.path.join(out_dir, "phase.txt"), "wb")
    records, stop, step = [], None, 0
    try:
        while True:
            sums = np.asarray(_call(api, "observe", m.observe)(num_pes, model, state, s["mass"], *tail), dtype=np.float64)
            rec = m.unpack(sums, num_pes, n_traj, *tail[1:])
            rec["t"] = step * dt
            if grid is not None:
                acc = (api.hop_bin_mf if amplitude else api.hop_bin)(num_pes, model, state, grid)
                if bandwidth is not None:
                    rho, (rec["smoothed"], rec["nonfinite"]) = (api.hop_smooth_mf if amplitude else api.hop_smooth)(num_pes, model, state, grid, bandwidth, n_traj)
                if files:
                    if bandwidth is None:
                        rho = (api.hop_density_mf if amplitude else api.hop_density)(num_pes, grid, acc, n_traj)
                    files["phase.txt"].write(exact.phase_text(api, rho[None]) if hasattr(api, "format_g") else exact.phase_block(rho).encode())
                if hasattr(acc, "is_cuda"):
                    api.synchronize()  # the context's stream has written acc: now the framework's may read it
                few = (acc[:num_pes * grid[2] * grid[5]].reshape(num_pes, -1).sum(1), acc[-2:])  # the only numbers of acc that cross
                if hasattr(acc, "is_cuda"):
                    few = tuple(v.cpu().numpy() for v in few)
                rec["binned"], rec["outside"] = (int(v) for v in few[1])
                if amplitude:
                    rec["binned_weights"] = np.asarray(few[0], dtype=np.float64) / 4294967296.0
                else:
                    rec["binned_counts"] = few[0]
            records.append(rec)
            if files:
                files["t.txt"].write(exact.fmt(rec["t"]) + "\n")
                files["averages.txt"].write(m.line(rec["t"], rec, n_traj))
            if m.running(sums, num_pes) == 0:
                stop = f"NO TRAJECTORY IS RUNNING, STOP EVOLVING AT {rec['t']:g}"
                break
            if step + output_step > total_step or (max_outputs is not None and len(records) >= max_outputs):
                break
            args, keywords = m.step_args(seed, reverse_frustrated, correction, tail, s["mass"], dt, step, output_step, s["xmin"], s["xmax"])
            state = _call(api, "evolve", m.evolve)(num_pes, model, state, *args, **keywords)
            step += output_step
    finally:
        for f in files.values():
            f.close()
    scattered, n_f, last = m.channels(sums, num_pes, n_traj)
    left = {}
    for axis, grid in outgoing_grids(api, num_pes, model, s, surface0, request).items():
        acc = _call(api, "outgoing", m.observe)(num_pes, model, state, s["mass"], grid, axis, *tail)
        if hasattr(acc, "is_cuda"):
            api.synchronize()  # the context's stream has written acc: now the framework's may read it
        density, tallies = outgoing_density(acc, num_pes, grid[2], max(float(n_f), 1.0), grid[1])  # an empty sample: every sum is 0
        left[axis] = dict(grid=grid, density=density, acc=acc, tallies=dict(zip(("binned", "outside", "running", "unassigned"), tallies)))
        if out_dir is not None:
            write_outgoing(out_dir, axis, grid, density)
    t_end = time.perf_counter()
    say(stop or "FINISHED ALL OUTPUT TIMES")
    line = " ".join(exact.fmt(v) for v in [_head(model, s), *scattered.reshape(-1), m.running(sums, num_pes) / n_traj, *last])
    result = m.result(dict(setup=s, dt=dt, output_step=output_step, total_step=total_step, n_traj=n_traj, records=records, stop=stop, state=state,
                           scattered=scattered, scattering_line=line, stop_time=records[-1]["t"], steps=step, total_seconds=t_end - t0,
                           decoherence=decoherence, edc_c=edc_c, method=method, phase_density=phase_density), tail, n_f, last)
    if bandwidth is not None:
        result = dict(result, phase_smooth=bandwidth)
    return dict(result, outgoing=left) if request else result


def scan_line(values):
    """One line of scan.txt: the head, the fractions [left | right][surface], the fraction running, their standard errors, hops and frustrated
    hops per trajectory, the drift of the mean energy"""
    return " ".join(exact.fmt(v) for v in values) + "\n"


def _per_group(setup_kw, n_groups):
    """setup_kw for every group: a list, tuple or array of n_groups values is one value per group, anything else is shared"""
    per = [dict() for _ in range(n_groups)]
    for key, value in setup_kw.items():
        many = isinstance(value, (list, tuple, np.ndarray))
        if many and len(value) != n_groups:
            raise ValueError(f"{key} has {len(value)} values for {n_groups} groups")
        for g in range(n_groups):
            per[g][key] = value[g] if many else value
    return per


def scan(api, model=DAC, num_pes=2, ln_energies=None, momenta=None, n_per_group=10000, seed=0, fixed=True, surface0=0, dt=None, chunk_steps=4096,
         max_steps=None, reverse_frustrated=False, out_dir=None, log=None, decoherence=None, edc_c=0.1, method="fssh", window=None, gamma=None, **setup_kw):
    """The branching probabilities as a function of the incoming momentum, Tully's plot, from ONE ensemble of len(ln_energies) (or len(momenta))
    groups of n_per_group trajectories.  Group g takes its constants from exact.setup(ln_energies[g], boundary=ABSORBING, **setup_kw) (momenta:
    p0 = momenta[g] instead): x0, p0, mass, the bounds xmin and xmax, its time step dt_rule unless dt (a number, or one per group) overrides
    it, and total_step = int(total_time / dt).  A list, tuple or array in setup_kw is one value per group.  mass, xmin and xmax must not differ
    between groups (ValueError).  fixed=True is Tully's convention, sigma_x = sigma_p = 0: every trajectory of a point starts at x0 with
    exactly p0, which is also what an energy-resolved exact curve (exact.run(spectrum=...)) is to be compared with; fixed=False draws from the
    setup's packet.  The ensemble stays on the device: one hop_sample_groups, then hop_evolve_groups in launches of chunk_steps steps (which
    bounds the length of one launch; the result does not depend on it, bit for bit), each followed by one hop_observe_groups, whose n_groups
    rows are all that crosses.  It stops when no trajectory of any group runs, else at max_steps (default: the largest total_step).
    decoherence and edc_c: as run(); with None hop_evolve_groups is called without these keywords, otherwise both are forwarded to every call.
    Returns per group (arrays with n_groups rows): head (ln E for DAC, else p0, as run()), scattered (n_groups, 2, num_pes) the fractions
    [left | right][surface], running, stderr (n_groups, 2 num_pes + 1) = sqrt(f (1 - f) / n_per_group) of those fractions in scan.txt's order,
    hops and frustrated per trajectory, energy_drift = (sum E_end - sum E_start) / n_per_group, and lines (scan_line, what scan.txt holds with
    out_dir); also setups, dt, steps, stop, state, hop_counts (the (n, 2) counters), rows (the last hop_observe_groups), decoherence and edc_c.
    method: "fssh" (the default: everything above, call for call) or "ehrenfest": the same sample, then hop_evolve_groups_mf and
    hop_observe_groups_mf.  scan.txt keeps its columns: the fractions are weights[left | right][k] / n_per_group and n_status[0] / n_per_group,
    hops and frustrated are 0 (hop_counts is None), energy_drift comes from the mean-field energy p^2 / 2m + sum_k |c_k|^2 E_k.  stderr is then
    an UPPER BOUND: a fraction f is the mean of weights in [0, 1], whose variance is at most f (1 - f).  With fixed=True every trajectory of a
    group is the same trajectory (nothing is random), so n_per_group = 1 is enough.  decoherence or reverse_frustrated=True with "ehrenfest" is
    a ValueError.  method "sqc" with window and gamma as run(), on hop_sample_groups_sqc, hop_evolve_groups_sqc and hop_observe_groups_sqc: channel
    (side, k) = counts[side][k] / N_f per group (0 where N_f = 0) with stderr sqrt(f (1 - f) / N_f), running = n_status[0] / n_per_group with stderr
    over n_per_group, hops and frustrated 0, energy_drift from H, and the unassigned fraction of the group's finished trajectories as a new last
    column of scan.txt.  method "mash": everything of "fssh"
    (scan.txt, the counters of hops taken and frustrated) on hop_sample_groups_mash and hop_evolve_groups_mash; the options run() refuses with it
    are a ValueError here too."""
    m = _method(method, decoherence, reverse_frustrated, None, window, gamma, num_pes)
    tail = sqc_window(window, gamma) if m.windowed else ()  # what follows surface0 in the sample and mass in the observe
    if (ln_energies is None) == (momenta is None):
        raise ValueError("give ln_energies or momenta, one of them")
    given = np.atleast_1d(np.asarray(ln_energies if momenta is None else momenta, dtype=np.float64))
    num_pes, n_groups, n_per_group, chunk_steps = int(num_pes), len(given), int(n_per_group), int(chunk_steps)
    if given.ndim != 1 or n_groups < 1 or n_per_group < 1 or chunk_steps < 1:
        raise ValueError("a scan has at least one group, one trajectory per group and one step per launch")
    setup_kw["boundary"] = exact.ABSORBING
    setups = []
    for v, kw in zip(given, _per_group(setup_kw, n_groups)):
        if momenta is not None:
            kw["p0"] = float(v)
        setups.append(exact.setup(float(v) if momenta is None else 0.0, **kw))
    s0 = setups[0]
    for key in ("mass", "xmin", "xmax"):
        if any(s[key] != s0[key] for s in setups):
            raise ValueError(f"the groups of a scan share one {key}")
    dts = np.array([s["dt_rule"] for s in setups]) if dt is None else np.broadcast_to(np.asarray(dt, dtype=np.float64), (n_groups,)).copy()
    total_step = [int(s["total_time"] / t) for s, t in zip(setups, dts)]
    max_steps = max(total_step) if max_steps is None else int(max_steps)
    packets = np.array([[s["x0"], s["p0"], 0.0 if fixed else s["sigma_x"], 0.0 if fixed else s["sigma_p"]] for s in setups])
    correction = {} if decoherence is None else dict(decoherence=decoherence, edc_c=edc_c)
    say = log or (lambda *_: None)
    t0 = time.perf_counter()
    state = _call(api, "sample", m.sample, True)(num_pes, model, n_per_group, seed, packets, surface0, *tail, device_out=True)
    on_device = hasattr(state[0], "is_cuda")
    if not m.counters:
        counts = None
    elif on_device:
        import torch
        counts = torch.zeros((n_groups * n_per_group, 2), dtype=torch.int32, device=state[0].device)
        torch.cuda.synchronize(state[0].device)  # the framework's stream has cleared the counters: now the context's may add to them
    else:
        counts = np.zeros((n_groups * n_per_group, 2), dtype=np.int32)
    width, step, stop = m.width(num_pes), 0, None

    def observe():
        sums = _call(api, "observe", m.observe, True)(num_pes, model, state, n_per_group, s0["mass"], *tail)
        return np.asarray(sums, dtype=np.float64).reshape(n_groups, width)

    first = rows = observe()
    while True:
        if m.running(rows, num_pes).sum() == 0:
            stop = f"NO TRAJECTORY IS RUNNING, STOP EVOLVING AT STEP {step}"
            break
        if step >= max_steps:
            break
        n_steps = min(chunk_steps, max_steps - step)
        args, keywords = m.step_args(seed, reverse_frustrated, correction, tail, s0["mass"], dts, step, n_steps, s0["xmin"], s0["xmax"])
        if m.counters:
            state, counts = _call(api, "evolve", m.evolve, True)(num_pes, model, state, n_per_group, *args, hops=counts, **keywords)
        else:
            state = _call(api, "evolve", m.evolve, True)(num_pes, model, state, n_per_group, *args, **keywords)
        step += n_steps
        rows = observe()
    if not m.counters:
        per_group = np.zeros((n_groups, 2), dtype=np.int64)
    elif on_device:
        api.synchronize()  # the context's stream has written the counters: now the framework's may read them
        per_group = counts.reshape(n_groups, n_per_group, 2).sum(dim=1, dtype=torch.int64).cpu().numpy()
    else:
        per_group = counts.reshape(n_groups, n_per_group, 2).sum(axis=1, dtype=np.int64)
    t_end = time.perf_counter()
    say(stop or f"STOPPED AT {max_steps} STEPS")
    scattered, n_f, last = m.channels(rows, num_pes, n_per_group)
    running = m.running(rows, num_pes) / n_per_group
    channels = scattered.reshape(n_groups, 2 * num_pes)
    spread = channels * (1.0 - channels)
    stderr = np.concatenate([np.sqrt(np.divide(spread, n_f[:, None], out=np.zeros_like(spread), where=n_f[:, None] > 0)),
                             np.sqrt(running * (1.0 - running) / n_per_group)[:, None]], axis=1)
    fractions = np.concatenate([channels, running[:, None]], axis=1)
    head = np.array([_head(model, s) for s in setups])
    hops, frustrated = per_group[:, 0] / n_per_group, per_group[:, 1] / n_per_group
    drift = (rows[:, width - 1] - first[:, width - 1]) / n_per_group
    lines = [scan_line([head[g], *fractions[g], *stderr[g], hops[g], frustrated[g], drift[g], *(column[g] for column in last)]) for g in range(n_groups)]
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "scan.txt"), "w") as f:
            f.write("".join(lines))
    return m.result(dict(setups=setups, dt=dts, n_per_group=n_per_group, total_step=total_step, max_steps=max_steps, steps=step, stop=stop, state=state,
                         hop_counts=counts, rows=rows, head=head, scattered=scattered, running=running, stderr=stderr, hops=hops, frustrated=frustrated,
                         energy_drift=drift, lines=lines, total_seconds=t_end - t0, decoherence=decoherence, edc_c=edc_c, method=method), tail, n_f, last)
