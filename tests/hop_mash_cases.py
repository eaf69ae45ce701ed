"""The cases of tests/test_gpu_hop_mash.py on the numpy restatement tests/hop_mash_numpy.py, each computed once per process: the two-level cases of
tests/test_gpu_hop.py with 293 trajectories (a tail that is no multiple of 64 or 256), seed 0, x0 = -4, sigma_p = p0 / 20, sigma_x = 1 / (2 sigma_p),
bounds +-6, mass 2000.  tests/test_hop_mash_host.py confirms without a GPU that the restatement alone sets no trajectory of them aside."""
import functools

import numpy as np

from gaussian_process_liouville_equation_amd import pes
from tests import hop_mash_numpy as HA
from tests import hop_numpy as HN

N_TRAJ, X0, MASS, LEFT, RIGHT, SEED = 293, -4.0, 2000.0, -6.0, 6.0, 0

# name: model (an id, or the built-in that is tabulated at dx = 1 / 16), p0, dt, steps, start surface
CASES = {
    "sac": dict(model=HN.SAC, p0=10.0, dt=2.0, steps=400),
    "dac16": dict(model=HN.DAC, p0=16.0, dt=1.0, steps=500),
    "dac10": dict(model=HN.DAC, p0=10.0, dt=2.0, steps=900),                 # frustrated hops, reflection
    "ecr": dict(model=HN.ECR, p0=10.0, dt=4.0, steps=700, surface0=1),       # from the upper surface
    "table2": dict(model=HN.DAC, p0=16.0, dt=1.0, steps=500, tabulated=True),
}


def widen(state):
    x, p, b, surface, status = state
    return x.astype(np.longdouble), p.astype(np.longdouble), b.astype(np.clongdouble), surface, status


def packet(p0):
    return X0, p0, 1.0 / (2.0 * p0 / 20.0), p0 / 20.0


@functools.lru_cache(maxsize=None)
def tabulated(model):
    """pes.tabulate of a built-in two-level model on [-8, 8] at dx = 1 / 16"""
    return HN.FunctionTable(*pes.tabulate(HN.scalar_function(HN.builtin(model, 2)), -8.0, 1.0 / 16.0, 257))


@functools.lru_cache(maxsize=None)
def reference(name):
    """The case on the restatement, once: the float64 sample (and D of its b), its evolution in float64 (with diagnostics) and in long double, D per
    quantity, and the trajectories the float64 restatement's own margins set aside"""
    assert np.finfo(np.longdouble).eps < 1e-18  # or D calibrates nothing
    c = {"surface0": 0, "tabulated": False, **CASES[name]}
    pot = HN.table(tabulated(c["model"])) if c["tabulated"] else HN.builtin(c["model"], 2)
    start = HA.sample(pot, 2, N_TRAJ, SEED, *packet(c["p0"]), c["surface0"])
    wide_start = HA.sample(pot, 2, N_TRAJ, SEED, *packet(c["p0"]), c["surface0"], dtype=np.longdouble)
    end, diag = HA.evolve(pot, start, MASS, c["dt"], c["steps"], LEFT, RIGHT)
    wide, wide_diag = HA.evolve(pot, widen(start), MASS, c["dt"], c["steps"], LEFT, RIGHT)
    aside = HA.set_aside(diag)
    keep = ~aside
    assert np.array_equal(end[3][keep], wide[3][keep]) and np.array_equal(end[4][keep], wide[4][keep])
    assert np.array_equal(diag["hops"][keep], wide_diag["hops"][keep]) and np.array_equal(diag["frustrated"][keep], wide_diag["frustrated"][keep])
    D = [float(np.abs(end[q] - wide[q])[keep].max()) for q in range(3)]
    return dict(case=c, potential=pot, start=start, end=end, diag=diag, D=D, aside=aside, D_sample=float(np.abs(start[2] - wide_start[2]).max()))
