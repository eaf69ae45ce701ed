"""Time of the sort of the finished trajectories into their channels (gple_hop_outgoing and its _mf and _sqc forms; DESIGN.md §17, "What left the
box") beside the scatter of the same state into phase space (gple_hop_bin with GPLE_HOP_BIN_ALL), in one process: GPLE_TIMER_HOP_OUTGOING and
GPLE_TIMER_HOP_BIN, each the bin kernel alone, as the median (min - max) over calls after a warm-up call, taken in turn.  DAC at two levels,
256 bins over p in [-32, 32] (or over the energies of the packet) against the 256 x 256 grid over x in [-8, 8] and the same p.  Two ensembles:
    finished   p0 = 10, x0 = -4, bounds +-6, dt = 2, `--steps` fewest-switches steps: what a finished run leaves
    crowd      every trajectory at one point of phase space, gone to the right on surface 1: every add of a call goes to one word
Prints one JSON line.

    python probes/hop_outgoing_timing.py [--trajectories 1048576] [--steps 1500] [--reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gaussian_process_liouville_equation_amd as pkg  # noqa: E402
from gaussian_process_liouville_equation_amd import _capi  # noqa: E402

MASS, X0, P0, DT, BOUND, SEED, DAC, BINS = 2000.0, -4.0, 10.0, 2.0, 6.0, 7, 1, 256
PHASE = (-8.0, 16.0 / (BINS - 1), BINS, -32.0, 64.0 / (BINS - 1), BINS)
MOMENTUM = PHASE[3:]
ENERGY = (-0.02, 0.12 / (BINS - 1), BINS)  # p^2 / 2m + E_a of the packet lies near 0.025


def spread(ms):
    return dict(ms=float(np.median(ms)), ms_min=min(ms), ms_max=max(ms))


def crowd(api, n):
    import torch

    where = torch.device("cuda", api.device)
    b = torch.zeros((n, 2), dtype=torch.complex128, device=where)
    b[:, 0] = 1.0
    state = (torch.full((n,), 7.0, dtype=torch.float64, device=where), torch.full((n,), 11.0, dtype=torch.float64, device=where), b,
             torch.ones(n, dtype=torch.int32, device=where), torch.full((n,), 2, dtype=torch.int32, device=where))
    torch.cuda.synchronize(where)
    return state


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trajectories", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=1500)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    api = pkg.open_api(0)
    api.enable_timing(True)
    rows = []
    try:
        finished = api.hop_sample(2, DAC, a.trajectories, SEED, X0, P0, 1.0 / (2.0 * P0 / 20.0), P0 / 20.0, 0, device_out=True)
        finished = api.hop_evolve(2, DAC, finished, SEED, MASS, DT, 0, a.steps, -BOUND, BOUND)
        api.synchronize()
        calls = {
            "surface momentum": lambda s: api.hop_outgoing(2, DAC, s, MASS, MOMENTUM, "momentum"),
            "surface energy": lambda s: api.hop_outgoing(2, DAC, s, MASS, ENERGY, "energy"),
            "amplitude momentum": lambda s: api.hop_outgoing_mf(2, DAC, s, MASS, MOMENTUM, "momentum"),
            "window momentum": lambda s: api.hop_outgoing_sqc(2, DAC, s, MASS, MOMENTUM, "momentum", "triangle"),
        }
        for ensemble, state in (("finished", finished), ("crowd", crowd(api, a.trajectories))):
            for label, call in calls.items():
                bin_ms, out_ms = [], []
                for k in range(1 + a.reps):  # call 0 of either warms up; the two take turns
                    mixed = api.hop_bin(2, DAC, state, PHASE, bin_all=True)
                    last = api.timing(_capi.TIMER_HOP_BIN)[0]
                    acc = call(state)
                    last_out = api.timing(_capi.TIMER_HOP_OUTGOING)[0]
                    if k:
                        bin_ms.append(last)
                        out_ms.append(last_out)
                acc, mixed = acc.cpu().numpy(), mixed.cpu().numpy()
                words = acc[:-4]
                assert acc[-4:].sum() == a.trajectories and mixed[-2:].sum() == a.trajectories
                one, two = spread(bin_ms), spread(out_ms)
                rows.append(dict(ensemble=ensemble, call=label, bin_ms=one["ms"], bin_ms_min=one["ms_min"], bin_ms_max=one["ms_max"], outgoing_ms=two["ms"],
                                 outgoing_ms_min=two["ms_min"], outgoing_ms_max=two["ms_max"], ratio=two["ms"] / one["ms"],
                                 within_bin_spread=bool(two["ms"] <= one["ms"] + (one["ms_max"] - one["ms_min"])), tallies=[int(v) for v in acc[-4:]],
                                 words_hit=int((words != 0).sum()), fullest_word=float(words.max() / 4294967296.0), bin_tallies=[int(v) for v in mixed[-2:]]))
    finally:
        api.close()
    print(json.dumps(dict(probe="hop_outgoing_timing", trajectories=a.trajectories, steps=a.steps, reps=a.reps, rows=rows)))


if __name__ == "__main__":
    main()
