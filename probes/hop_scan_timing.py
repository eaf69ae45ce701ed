"""A momentum scan as one grouped ensemble against the loop a user writes without the grouped calls ("A curve in one launch").
One process, 64 groups x 16384 fixed-momentum DAC trajectories (2^20 in all; p0 uniform in [10, 30], x0 = -4, dt = 1, mass 2000), 1000 steps,
bounds far away, so every trajectory runs every step:

  kernel   GPLE_TIMER_HOP_GROUPS of one gple_hop_evolve_groups call, median of --reps calls after a warm-up call (min - max), every call from a
           fresh sample, as trajectory-steps per second; GPLE_TIMER_HOP of gple_hop_evolve over the same 2^20 trajectories (one packet, the
           plain figure of probes/hop_timing.py) measured the same way in the same process beside it
  scan     the wall time of one scan: gple_hop_sample_groups, gple_hop_evolve_groups (with the hop counters), gple_hop_observe_groups, the rows
           on the host; against the same 64 groups as 64 sequences gple_hop_sample / gple_hop_evolve / gple_hop_observe of 16384 trajectories
           with their offsets through the plain entry points (sigma = 1e-300: the plain sample refuses 0), what a user writes on the parent.
           Median of --reps after a warm-up each, alternated

Prints one JSON line.

    python probes/hop_scan_timing.py [--groups 64] [--per-group 16384] [--steps 1000] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gaussian_process_liouville_equation_amd as pkg  # noqa: E402
from gaussian_process_liouville_equation_amd import _capi  # noqa: E402

TIMER_HOP = 12
DAC, MASS, X0, DT, FAR, SEED = 1, 2000.0, -4.0, 1.0, 1e6, 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=64)
    ap.add_argument("--per-group", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    G, per, n = a.groups, a.per_group, a.groups * a.per_group
    p0 = np.linspace(10.0, 30.0, G)
    packets = np.stack([np.full(G, X0), p0, np.zeros(G), np.zeros(G)], axis=1)
    dts = np.full(G, DT)
    api = pkg.open_api(0)
    api.enable_timing(True)
    try:
        import torch

        kernel = {"groups": [], "plain": []}
        for k in range(1 + a.reps):  # call 0 warms up
            state = api.hop_sample_groups(2, DAC, per, SEED, packets, device_out=True)
            state = api.hop_evolve_groups(2, DAC, state, per, SEED, MASS, dts, 0, a.steps, -FAR, FAR)
            ms_groups = api.timing(_capi.TIMER_HOP_GROUPS)[0]
            rows = api.hop_observe_groups(2, DAC, state, per, MASS)
            assert rows[:, :2].sum() == n  # every trajectory ran to the end
            state = api.hop_sample(2, DAC, n, SEED, X0, 16.0, 0.625, 0.8, device_out=True)
            state = api.hop_evolve(2, DAC, state, SEED, MASS, DT, 0, a.steps, -FAR, FAR)
            ms_plain = api.timing(TIMER_HOP)[0]
            if k:
                kernel["groups"].append(ms_groups)
                kernel["plain"].append(ms_plain)

        def scan():
            state = api.hop_sample_groups(2, DAC, per, SEED, packets, device_out=True)
            counts = torch.zeros((n, 2), dtype=torch.int32, device=state[0].device)
            torch.cuda.synchronize(state[0].device)
            state, counts = api.hop_evolve_groups(2, DAC, state, per, SEED, MASS, dts, 0, a.steps, -FAR, FAR, hops=counts)
            return api.hop_observe_groups(2, DAC, state, per, MASS)

        def loop():
            rows = []
            for g in range(G):
                state = api.hop_sample(2, DAC, per, SEED, X0, p0[g], 1e-300, 1e-300, trajectory_offset=g * per, device_out=True)
                state = api.hop_evolve(2, DAC, state, SEED, MASS, DT, 0, a.steps, -FAR, FAR, trajectory_offset=g * per)
                rows.append(api.hop_observe(2, DAC, state, MASS))
            return np.array(rows)

        wall = {"scan": [], "loop": []}
        for k in range(1 + a.reps):
            for name, fun in (("scan", scan), ("loop", loop)):
                api.synchronize()
                t0 = time.perf_counter()
                out = fun()
                seconds = time.perf_counter() - t0
                assert out[:, :2].sum() == n
                if k:
                    wall[name].append(seconds)
        row = lambda v, scale=1.0: dict(median=float(np.median(v)) * scale, min=min(v) * scale, max=max(v) * scale)
        result = dict(probe="hop_scan_timing", groups=G, per_group=per, steps=a.steps, reps=a.reps,
                      kernel_ms_groups=row(kernel["groups"]), kernel_ms_plain=row(kernel["plain"]),
                      trajectory_steps_per_second_groups=n * a.steps / (float(np.median(kernel["groups"])) * 1e-3),
                      trajectory_steps_per_second_plain=n * a.steps / (float(np.median(kernel["plain"])) * 1e-3),
                      wall_ms_scan=row(wall["scan"], 1e3), wall_ms_loop=row(wall["loop"], 1e3),
                      loop_over_scan=float(np.median(wall["loop"]) / np.median(wall["scan"])))
    finally:
        api.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
