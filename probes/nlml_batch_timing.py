"""Timing of the batched NLML evaluation and of the lock-step search on it (gple_nlml_batch, gple_nlml_fit_planes) against
the routes the library had before them, in the same process: B calls of gple_nlml one after another, and reconstruct.optimize plane by plane.
Wall time of the calls as the driver makes them (host arrays in, results out — launch, synchronisation and callback latency are what the
batch removes, so device events alone would miss the point); the two routes alternate, medians of --reps after a warm-up.  Prints the two
markdown tables of §13.

    python probes/nlml_batch_timing.py [--sizes 64,200,256] [--batches 1,4,9,16,36,144] [--planes 4] [--maxeval 0] [--reps 5]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gaussian_process_liouville_equation_amd as pkg  # noqa: E402
from gaussian_process_liouville_equation_amd import reconstruct  # noqa: E402

HYPER = np.array([0.1, 1.2, 1.0 / 0.8, 1.0 / 0.7])
LOWER, UPPER = np.array([1e-3, 1e-2, 0.05, 0.05]), np.array([1.0, 10.0, reconstruct.DBL_MAX, reconstruct.DBL_MAX])


def packet(N, seed):
    """N samples of a Gaussian wave packet with its density as labels"""
    rng = np.random.Generator(np.random.PCG64(seed))
    X = rng.normal([-10.0, 14.112], [0.7086, 0.7056], size=(N, 2))
    y = np.exp(-0.5 * (((X[:, 0] + 10.0) / 0.7086) ** 2 + ((X[:, 1] - 14.112) / 0.7056) ** 2)) / (2 * np.pi * 0.7086 * 0.7056)
    return np.ascontiguousarray(X), y


def alternate(old, new, reps):
    """median wall milliseconds of old() and new(), run in turn (round 0 warms up)"""
    ms = ([], [])
    for k in range(reps + 1):
        for which, fn in enumerate((old, new)):
            t0 = time.perf_counter()
            fn()
            if k:
                ms[which].append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ms[0])), float(np.median(ms[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,200,256")
    ap.add_argument("--batches", default="1,4,9,16,36,144")
    ap.add_argument("--planes", type=int, default=4)
    ap.add_argument("--maxeval", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    api = pkg.open_api(0)
    sizes = [int(v) for v in a.sizes.split(",")]
    print("| N | B | B x gple_nlml value ms | gple_nlml_batch value ms | ratio | B x gple_nlml value + gradient ms | gple_nlml_batch value + gradient ms | ratio | batch us per problem |")
    print("|---|---|---|---|---|---|---|---|---|")
    for N in sizes:
        for B in [int(v) for v in a.batches.split(",")]:
            sets = [packet(N, 100 * N + b) for b in range(B)]
            Xs, ys, xs = [s[0] for s in sets], [s[1] for s in sets], [HYPER] * B
            row = []
            for want_grad in (False, True):
                old, new = alternate(lambda: [api.nlml(HYPER, X, y, want_grad=want_grad) for X, y in sets],
                                     lambda: api.nlml_batch(xs, Xs, ys, want_grad=want_grad), a.reps)
                row += [old, new, old / new]
            print(f"| {N} | {B} | {row[0]:.3f} | {row[1]:.3f} | {row[2]:.2f} | {row[3]:.3f} | {row[4]:.3f} | {row[5]:.2f} | {1e3 * row[4] / B:.1f} |", flush=True)
    print(f"\n| N | planes | optimize plane by plane ms | evaluations | gple_nlml_fit_planes ms | evaluations | serial / batched |")
    print("|---|---|---|---|---|---|---|")
    for N in sizes:
        sets = [packet(N, 7000 + 10 * N + q) for q in range(a.planes)]
        counts = {}

        def serial():
            counts["serial"] = sum(reconstruct.optimize(api, X, y, HYPER, LOWER, UPPER, a.maxeval)[2] for X, y in sets)

        def batched():
            counts["batched"] = int(reconstruct.optimize_planes(api, sets, [HYPER] * a.planes, [LOWER] * a.planes, [UPPER] * a.planes, a.maxeval)[2].sum())

        old, new = alternate(serial, batched, a.reps)
        print(f"| {N} | {a.planes} | {old:.1f} | {counts['serial']} | {new:.1f} | {counts['batched']} | {old / new:.2f} |", flush=True)
    api.close()


if __name__ == "__main__":
    main()
