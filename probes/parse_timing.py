"""Timing of reading one output time of phase.txt (gple_parse_g) against the host route of the same pull of reconstruct.run_files:
a random (2, 2, n, n) complex state is written as one block of a phase.txt by gple_format_g, then read back file -> device-resident state on
both routes — device: reconstruct.phase_blocks, upload of the bytes, Api.parse_g(device_out=True); host: float() per token into numpy, then the
upload of the state — median of --reps after a warm-up, alternated in one process.  Also GPLE_TIMER_PARSE of the converting call (numbers
per second) beside the host-to-device time of the text.  Prints the markdown table of §15.

    python probes/parse_timing.py [--sizes 481,1921] [--reps 5] [--dir DIR]
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import gaussian_process_liouville_equation_amd as pkg  # noqa: E402
from gaussian_process_liouville_equation_amd import reconstruct  # noqa: E402

TIMER_PARSE = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="481,1921")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dir", default=None)
    args = ap.parse_args()
    api = pkg.open_api(0)
    rows = []
    try:
        with tempfile.TemporaryDirectory(dir=args.dir) as tmp:
            for n in (int(v) for v in args.sizes.split(",")):
                rng = np.random.default_rng(n)
                rho = torch.from_numpy(rng.normal(size=(2, 2, n, n, 2)) * 10.0 ** rng.uniform(-12, 0, size=(2, 2, n, n, 2))).cuda()
                path = os.path.join(tmp, f"phase_{n}.txt")
                with open(path, "wb") as f:
                    f.write(api.format_g(rho, 2 * n * n, 4))
                count = rho.numel()

                def device_route():
                    (block,) = reconstruct.phase_blocks(path, 2, n, n)
                    values, lines = api.parse_g(block, device_out=True)
                    assert len(values) == count and lines == 4
                    return values

                def host_route():
                    (block,) = reconstruct.phase_blocks(path, 2, n, n)
                    values, lines = reconstruct._parse_host(block)
                    assert len(values) == count and lines == 4
                    values = torch.from_numpy(values).cuda()
                    torch.cuda.synchronize()
                    return values

                assert torch.equal(device_route(), host_route())  # warm-up, and the same bits
                dev, host = [], []
                for _ in range(args.reps):
                    for route, out in ((device_route, dev), (host_route, host)):
                        t0 = time.perf_counter()
                        route()
                        out.append(time.perf_counter() - t0)
                # the kernels alone, beside the upload of the text
                (block,) = reconstruct.phase_blocks(path, 2, n, n)
                text = torch.frombuffer(block, dtype=torch.uint8)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                dtext = text.cuda()
                torch.cuda.synchronize()
                h2d = time.perf_counter() - t0
                api.enable_timing(True)
                kernel = []
                for _ in range(args.reps):
                    api.parse_g(dtext)
                    kernel.append(api.timing(TIMER_PARSE)[0] * 1e-3)
                api.enable_timing(False)
                rows.append((n, count, len(block), statistics.median(dev), statistics.median(host), statistics.median(kernel), h2d))
    finally:
        api.close()
    print("| n | numbers | text MB | device route s | host route s | ratio | GPLE_TIMER_PARSE ms (convert) | numbers / s | text H2D ms |")
    print("|---|---|---|---|---|---|---|---|---|")
    for n, count, length, d, h, k, c in rows:
        print(f"| {n} | {count} | {length / 1e6:.1f} | {d:.3f} | {h:.3f} | {h / d:.1f} | {1e3 * k:.2f} | {count / k:.3g} | {1e3 * c:.1f} |")


if __name__ == "__main__":
    main()
