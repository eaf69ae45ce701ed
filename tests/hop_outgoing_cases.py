"""The cases tests/test_gpu_hop_outgoing.py and tests/test_hop_outgoing_host.py share: ensembles of 293 trajectories (a tail that is no multiple
of 64 or 256), seed 0, x0 = -4, sigma_p = p0 / 20, sigma_x = 1 / (2 sigma_p), bounds +-6, mass 2000, as tests/hop_mash_cases.py, evolved until
trajectories have left on both sides where the model lets them and some still run.  A case has one ensemble per KIND: fewest switches
("surface" form), Ehrenfest ("amplitude"), SQC on the square and the triangle window ("window").  The GPU test evolves them on the device; here
they are evolved by the restatements, each once per process, for the host test."""
import functools

import numpy as np

from gaussian_process_liouville_equation_amd import pes
from tests import hop_mf_numpy as HM
from tests import hop_numpy as HN
from tests import hop_outgoing_numpy as HO
from tests import hop_sqc_numpy as HQ

N_TRAJ, X0, MASS, LEFT, RIGHT, SEED, N_BINS = 293, -4.0, 2000.0, -6.0, 6.0, 0, 64
EDGE, WINDOW_EDGE, MOST_ASIDE = 1e-9, 1e-10, 2  # set aside: a long double q_E this near (in steps) a cell edge, an e_k this near a window edge; the cap

CASES = {
    "dac10": dict(model=HN.DAC, N=2, p0=10.0, dt=2.0, steps=900),
    "tsac": dict(model=HN.TSAC, N=3, p0=10.0, dt=4.0, steps=550, surface0=1),
    "table2": dict(model=HN.DAC, N=2, p0=10.0, dt=2.0, steps=900, tabulated=True),
}
# kind: (the form of its outgoing call, the window code and gamma of an SQC ensemble)
KINDS = {"fssh": ("surface", None, None), "ehrenfest": ("amplitude", None, None), "square": ("window", HQ.SQUARE, 0.366),
         "triangle": ("window", HQ.TRIANGLE, 1.0 / 3.0)}


def packet(p0):
    return X0, p0, 1.0 / (2.0 * p0 / 20.0), p0 / 20.0


@functools.lru_cache(maxsize=None)
def tabulated(model, N):
    """pes.tabulate of a built-in model on [-8, 8] at dx = 1 / 16"""
    return HN.FunctionTable(*pes.tabulate(HN.scalar_function(HN.builtin(model, N)), -8.0, 1.0 / 16.0, 257))


def case_of(name):
    c = {"surface0": 0, "tabulated": False, **CASES[name]}
    c["potential"] = HN.table(tabulated(c["model"], c["N"])) if c["tabulated"] else HN.builtin(c["model"], c["N"])
    return c


@functools.lru_cache(maxsize=None)
def ensemble(name, kind):
    """the case's ensemble of that kind on the restatements"""
    c = case_of(name)
    pot, N = c["potential"], c["N"]
    _, window, gamma = KINDS[kind]
    if kind == "fssh":
        return HN.evolve(pot, HN.sample(pot, N, N_TRAJ, SEED, *packet(c["p0"]), c["surface0"]), SEED, MASS, c["dt"], 0, c["steps"], LEFT, RIGHT)[0]
    if kind == "ehrenfest":
        return HM.evolve(pot, HN.sample(pot, N, N_TRAJ, SEED, *packet(c["p0"]), c["surface0"]), MASS, c["dt"], c["steps"], LEFT, RIGHT)[0]
    return HQ.evolve(pot, HQ.sample(pot, N, N_TRAJ, SEED, *packet(c["p0"]), c["surface0"], window, gamma), MASS, c["dt"], c["steps"], LEFT, RIGHT, gamma)[0]


def momentum_grid(p0):
    """64 points over [-2 p0, 2 p0]: wide enough for what TSAC's lower surface gives back, and coarse enough for bins to collide"""
    return (-2.0 * p0, 4.0 * p0 / (N_BINS - 1), N_BINS)


def energy_grid(form, potential, state, window=None, gamma=None):
    """64 points of which the inner 62 span the energies of the finished trajectories: an input of the test made from the state it bins"""
    c = HO.classify(form, potential, state, MASS, window, gamma)
    q = c["energy"][c["finished"]].astype(np.float64)
    step = max(float(q.max() - q.min()), 1e-6) / (N_BINS - 3)
    return (float(q.min()) - step, step, N_BINS)


def set_aside(form, potential, state, grid, axis, window=None, gamma=None):
    """the trajectories the long double restatement sets aside for this call: a q_E within EDGE steps of a cell edge, and for the window form an
    e_k within WINDOW_EDGE of a window edge"""
    m = HO.margins(form, potential, state, MASS, grid, axis, window, gamma)
    return (m["edge"] <= EDGE) | (m["window"] <= WINDOW_EDGE), m
