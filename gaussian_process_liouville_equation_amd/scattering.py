"""Exact branching probabilities per energy: the coupled-channel Schrodinger equation on the library's diabatic potentials, solved on the device by
the renormalised Numerov method (gple_scatter, include/gple.h).  The exact line under every trajectory curve of hopping.scan.

    from gaussian_process_liouville_equation_amd import scattering
    r = scattering.run(api, model=scattering.SAC, momenta=np.linspace(3, 30, 256), x_left=-20, x_right=20, out_dir="out")
    r["scattered"]          # (n, 2, num_pes): [left | right][surface] from surface0, the order of scan.txt

The potential is taken to be constant beyond x_left and x_right: the box has to hold everything but the flat asymptotes.
"""
import os

import numpy as np

SAC, DAC, ECR, TSAC = 0, 1, 2, 3
HBAR = 1.0
KH_DEFAULT = 0.1  # the default grid: the smallest n_steps with k_max h <= 0.1


def end_energies(api, num_pes, model, x_left, x_right):
    """(2, num_pes): the ascending adiabatic energies of the potential at x_left and at x_right"""
    V, _ = api.pes_diabatic_n(num_pes, model, np.array([x_left, x_right], dtype=np.float64))
    return np.linalg.eigvalsh(np.asarray(V, dtype=np.float64))


def default_steps(e_max, lowest, mass, x_left, x_right, kh=KH_DEFAULT):
    """the smallest n_steps with k_max h <= kh, k_max = sqrt(2 m (e_max - lowest)) / hbar, at least 2"""
    k_max = np.sqrt(max(2.0 * mass * (e_max - lowest), 0.0)) / HBAR
    return max(2, int(np.ceil(k_max * (x_right - x_left) / kh)))


def smatrix_line_values(head, scattered, defect):
    """the numbers of the lines of smatrix.txt: the head, the 2 num_pes probabilities [left | right][surface], the defect"""
    n = len(head)
    return np.concatenate([np.asarray(head, dtype=np.float64)[:, None], np.asarray(scattered, dtype=np.float64).reshape(n, -1),
                           np.asarray(defect, dtype=np.float64)[:, None]], axis=1)


def run(api, model=DAC, num_pes=2, momenta=None, energies=None, surface0=0, x_left=-20.0, x_right=20.0, n_steps=None, richardson=False, out_dir=None,
        mass=2000.0):
    """The exact reflection and transmission probabilities per adiabatic surface for a particle coming in from the left on surface0, at every
    momentum of `momenta` (E = p^2 / 2m + eps_surface0(x_left)) or every total energy of `energies` (the potential's own zero), one of the two.
    One Api.scatter call for all of them (two with richardson=True).  n_steps: the grid; by default the smallest with k_max h <= 0.1, k_max from
    the largest energy and the lowest adiabatic energy of either end.  richardson=True solves on n_steps and 2 n_steps and returns
    (16 P_2N - P_N) / 15 (the method is fourth order) with |P_2N - P_N| as `error`.
    Returns: energies, momenta (NaN where surface0 is closed), head (ln(p^2 / 2m) for DAC, else p, as hopping.scan), prob (n, num_pes, 2, num_pes)
    every incoming surface, scattered (n, 2, num_pes) = prob[:, surface0], defect (n,) of surface0 (richardson: that of the 2 n_steps solution), error (richardson: as scattered, else None),
    n_steps, lines (what smatrix.txt holds with out_dir: per energy the head, the 2 num_pes probabilities in scan.txt's order
    [left | right][surface] and the defect, "%g" through api.format_g)."""
    if (momenta is None) == (energies is None):
        raise ValueError("give momenta or energies, one of them")
    num_pes, surface0, mass, x_left, x_right = int(num_pes), int(surface0), float(mass), float(x_left), float(x_right)
    if not 0 <= surface0 < num_pes:
        raise ValueError("surface0 is one of the num_pes surfaces")
    ends = end_energies(api, num_pes, model, x_left, x_right)
    e_in = float(ends[0, surface0])
    if momenta is not None:
        momenta = np.atleast_1d(np.asarray(momenta, dtype=np.float64))
        energies = momenta * momenta / 2.0 / mass + e_in
    else:
        energies = np.atleast_1d(np.asarray(energies, dtype=np.float64))
        with np.errstate(invalid="ignore"):
            momenta = np.sqrt(2.0 * mass * (energies - e_in))
    if energies.ndim != 1 or len(energies) < 1:
        raise ValueError("at least one momentum or energy, in one dimension")
    if n_steps is None:
        n_steps = default_steps(float(energies.max()), float(ends.min()), mass, x_left, x_right)
    n_steps = int(n_steps)
    prob, defect = api.scatter(num_pes, model, mass, x_left, x_right, n_steps, energies)
    prob, defect = np.asarray(prob, dtype=np.float64), np.asarray(defect, dtype=np.float64)
    error = None
    if richardson:
        fine, fine_defect = api.scatter(num_pes, model, mass, x_left, x_right, 2 * n_steps, energies)
        fine, defect = np.asarray(fine, dtype=np.float64), np.asarray(fine_defect, dtype=np.float64)
        full_error = np.abs(fine - prob)
        prob = (16.0 * fine - prob) / 15.0
        error = full_error[:, surface0]
    with np.errstate(invalid="ignore", divide="ignore"):
        head = np.log(momenta * momenta / 2.0 / mass) if model == DAC else momenta
    scattered, defect0 = prob[:, surface0], defect[:, surface0]
    values = smatrix_line_values(head, scattered, defect0)
    text = bytes(api.format_g(values, values.shape[1], join=True))
    lines = text.decode().splitlines(keepends=True)
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "smatrix.txt"), "wb") as f:
            f.write(text)
    return dict(energies=energies, momenta=momenta, head=head, prob=prob, scattered=scattered, defect=defect0, error=error, n_steps=n_steps, lines=lines,
                surface0=surface0, mass=mass, x_left=x_left, x_right=x_right)


def packet_rule(p0, sigma_p, n_points=129):
    """the uniform rule of packet_line: n_points momenta over p0 +- 6 sigma_p and their weights exp(-(p - p0)^2 / (2 sigma_p^2)), normalised to sum 1
    (sigma_p: the standard deviation of the packet's momentum density)"""
    p0, sigma_p, n_points = float(p0), float(sigma_p), int(n_points)
    if not (sigma_p > 0.0 and p0 - 6.0 * sigma_p > 0.0 and n_points >= 3):
        raise ValueError("sigma_p positive, p0 - 6 sigma_p positive and at least three points")
    p = np.linspace(p0 - 6.0 * sigma_p, p0 + 6.0 * sigma_p, n_points)
    t = (p - p0) / sigma_p
    w = np.exp(-0.5 * t * t)
    return p, w / w.sum()


def packet_line(api, model=DAC, num_pes=2, p0=10.0, sigma_p=0.5, surface0=0, x_left=-20.0, x_right=20.0, n_points=129, **run_kw):
    """What a Gaussian packet of mean momentum p0 and momentum spread sigma_p scatters into: the average of the exact columns over its momentum
    density on packet_rule's momenta, (2, num_pes) = [left | right][surface].  The figure to put beside the scattering line of exact.run(flux=True)
    and of hopping.run.  Every momentum of the rule has to be open on surface0 (else the average is NaN).  run_kw: mass, n_steps, richardson"""
    p, w = packet_rule(p0, sigma_p, n_points)
    r = run(api, model=model, num_pes=num_pes, momenta=p, surface0=surface0, x_left=x_left, x_right=x_right, **run_kw)
    return np.tensordot(w, r["scattered"], axes=(0, 0))
