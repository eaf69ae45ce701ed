"""Timing of the absorbed-population bookkeeping of the exact DVR dynamics (gple_dvr_flux / gple_dvr_flux_apply, csrc/gple_dvr_flux.hip;
DESIGN.md §11) at the ln E = 0 defaults of schrodinger_equation/input.py (n = 1935, dim 3870, output_step = 1280).  One JSON line per figure:
  flux      GPLE_TIMER_DVR_FLUX of one gple_dvr_flux call (median of --reps after a warm-up), the whole call, and by count the real-GEMM
            flops of the power (lower tiles) and of the sandwiches (four products on full tiles, four on lower tiles each), with the rate
            against the 78.6 TFLOP/s fp64 MFMA peak; GPLE_TIMER_DVR_POWER of gple_dvr_propagator on the same box beside it
  apply     one gple_dvr_flux_apply per state (T = 1), and per state in a call of 26 states
  e2e       seconds of `examples/exact_dvr.py 0 <dir> text absorbing flux` as a child process, and its last lines
    python probes/dvr_flux_timing.py [--reps 3] [--no-e2e] [--e2e-limit 600] [--ln-e 0]"""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gaussian_process_liouville_equation_amd as pkg  # noqa: E402
from gaussian_process_liouville_equation_amd import exact  # noqa: E402

PEAK = 78.6e12
TIMER_DVR_POWER, TIMER_DVR_FLUX = 9, 10


def flops(ld, s, channels, tile=64):
    """(power, sandwiches): real-GEMM flops by count.  A lower-tile product computes nt (nt + 1) / 2 tiles of ld^3 / nt^2 each"""
    nt = ld // tile
    full, lower = 2.0 * ld ** 3, 2.0 * tile * tile * ld * (nt * (nt + 1) // 2)
    squarings, multiplications = s.bit_length() - 1, bin(s)[3:].count("1")
    power = (6 + 4 * (squarings + multiplications)) * lower
    sandwiches = channels * (squarings + multiplications) * (4 * full + 4 * lower) + 4 * lower  # and the Hermitian product of L
    return power, sandwiches


def main():
    args = sys.argv[1:]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 3
    ln_e = float(args[args.index("--ln-e") + 1]) if "--ln-e" in args else 0.0
    e2e_limit = int(args[args.index("--e2e-limit") + 1]) if "--e2e-limit" in args else 600
    s = exact.setup(ln_e, boundary=exact.ABSORBING)
    n, dx, x, mass, steps = s["n_grids"], s["dx"], s["x"], s["mass"], s["output_step"]
    dim, ld = 2 * n, (2 * n + 63) // 64 * 64
    n_left = int(np.sum(x < (s["xmin"] + s["xmax"]) / 2.0))
    api = pkg.open_api(0)
    api.enable_timing(True)
    try:
        H, _, B = api.dvr_hamiltonian(2, exact.DAC, exact.REFLECTIVE, x[0], dx, n, mass)
        W = api.dvr_absorber(x[0], dx, n, mass, s["xmin"], s["xmax"], s["absorbing_length"])
        psi0 = exact.to_diabatic(exact.initial_adiabatic_psi(x, s["x0"], s["p0"], s["sigma_x"], 2), B)
        api.dvr_propagator(2, n, H, W, s["dt"], steps, device_out=True)  # warm-up
        power_ms = []
        for _ in range(reps):
            api.dvr_propagator(2, n, H, W, s["dt"], steps, device_out=True)
            power_ms.append(api.timing(TIMER_DVR_POWER)[0])
        U, G = api.dvr_flux(2, n, H, W, s["dt"], steps, B, n_left, device_out=True)  # warm-up
        ms, wall = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            U, G = api.dvr_flux(2, n, H, W, s["dt"], steps, B, n_left, device_out=True)
            wall.append(time.perf_counter() - t0)
            ms.append(api.timing(TIMER_DVR_FLUX)[0])
        f_power, f_sandwich = flops(ld, steps, 4)
        t_flux, t_power = float(np.median(ms)) * 1e-3, float(np.median(power_ms)) * 1e-3
        print(json.dumps(dict(figure="flux", dim=dim, ld=ld, n_steps=steps, n_left=n_left, flux_ms=1e3 * t_flux, call_s=float(np.median(wall)),
                              power_ms=1e3 * t_power, power_tflops=f_power / t_power / 1e12, tflop=(f_power + f_sandwich) / 1e12,
                              tflops=(f_power + f_sandwich) / t_flux / 1e12, sandwich_tflops=f_sandwich / (t_flux - t_power) / 1e12,
                              fraction_of_fp64_mfma_peak=(f_power + f_sandwich) / t_flux / PEAK, work_gbytes=8.0 * 21 * ld * ld / 1e9)), flush=True)
        api.dvr_flux_apply(2, n, G, psi0)
        t0 = time.perf_counter()
        for _ in range(10):
            one = api.dvr_flux_apply(2, n, G, psi0)
        t_one = (time.perf_counter() - t0) / 10
        psi = np.concatenate([psi0[None, :], api.dvr_apply(2, n, U, psi0, 25)])
        t0 = time.perf_counter()
        taken = api.dvr_flux_apply(2, n, G, psi)
        t_many = (time.perf_counter() - t0) / 26
        print(json.dumps(dict(figure="apply", s_per_state_alone=t_one, s_per_state_of_26=t_many, gbytes_of_g=64.0 * dim * dim / 1e9,
                              gbytes_per_s_alone=64.0 * dim * dim / 1e9 / t_one, same_bits=bool(np.array_equal(one[0], taken[0])),
                              absorbed_after_26_outputs=(taken.sum(axis=0) * dx).tolist())), flush=True)
    finally:
        api.close()
    if "--no-e2e" not in args:
        with tempfile.TemporaryDirectory() as out:
            t0 = time.perf_counter()
            try:
                r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "exact_dvr.py"), "%g" % ln_e, out, "text", "absorbing", "flux"],
                                   capture_output=True, text=True, timeout=e2e_limit)
                print(json.dumps(dict(figure="e2e", seconds=time.perf_counter() - t0, returncode=r.returncode, tail=r.stdout.strip().splitlines()[-5:],
                                      absorbed_txt_tail=open(os.path.join(out, "absorbed.txt")).read().splitlines()[-1:] if r.returncode == 0 else r.stderr[-400:])),
                      flush=True)
            except subprocess.TimeoutExpired:
                print(json.dumps(dict(figure="e2e", seconds=None, note="not finished within %d s" % e2e_limit)), flush=True)


if __name__ == "__main__":
    main()
