"""Timing of the absorbing boundary of the exact DVR dynamics (gple_dvr_propagator / gple_dvr_apply, csrc/gple_dvr_power.hip)
at the ln E = 0 defaults of schrodinger_equation/input.py (n = 1935, dim 3870, output_step = 1280).  One JSON line per figure on stdout:
  power     GPLE_TIMER_DVR_POWER of one gple_dvr_propagator call (median of --reps after a warm-up) and, by the count 3 Horner products of
            2 real GEMMs + (squarings + multiplications) of 4 real GEMMs, lower tiles only, its share of the 78.6 TFLOP/s fp64 MFMA peak
  stepping  the yardstick: output_step applications of the one-step propagator (n_steps = 1) through gple_dvr_apply — stepping at a quarter
            of RK4's true cost (one matrix-vector product per step instead of four), which is in stepping's favour
  apply     one application of U per output
  e2e       seconds of `examples/exact_dvr.py 0 <dir> text absorbing` as a child process
  return    how much population is back in the interior after the packet has left, against a reflective run in a wider box whose walls the
            packet has not reached by then (recorded, not asserted)
    python probes/dvr_absorbing_timing.py [--reps 3] [--no-e2e] [--e2e-limit 600] [--ln-e 0]"""
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
TIMER_DVR_POWER = 9


def power_flops(ld, s, tile=64):
    """real-GEMM flops of one propagator: the lower tiles (diagonal ones whole) of 3 x 2 + products x 4 products of ld^3"""
    nt = ld // tile
    per_gemm = 2.0 * tile * tile * ld * (nt * (nt + 1) // 2)
    products = (s.bit_length() - 1) + bin(s)[3:].count("1")
    return (6 + 4 * products) * per_gemm, products


def main():
    args = sys.argv[1:]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 3
    ln_e = float(args[args.index("--ln-e") + 1]) if "--ln-e" in args else 0.0
    e2e_limit = int(args[args.index("--e2e-limit") + 1]) if "--e2e-limit" in args else 600
    s = exact.setup(ln_e, boundary=exact.ABSORBING)
    n, dx, x, mass, steps = s["n_grids"], s["dx"], s["x"], s["mass"], s["output_step"]
    dim, ld = 2 * n, (2 * n + 63) // 64 * 64
    api = pkg.open_api(0)
    api.enable_timing(True)
    try:
        H, _, B = api.dvr_hamiltonian(2, exact.DAC, exact.REFLECTIVE, x[0], dx, n, mass)
        W = api.dvr_absorber(x[0], dx, n, mass, s["xmin"], s["xmax"], s["absorbing_length"])
        psi0 = exact.to_diabatic(exact.initial_adiabatic_psi(x, s["x0"], s["p0"], s["sigma_x"], 2), B)
        U = api.dvr_propagator(2, n, H, W, s["dt"], steps, device_out=True)  # warm-up
        ms, wall = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            U = api.dvr_propagator(2, n, H, W, s["dt"], steps, device_out=True)
            wall.append(time.perf_counter() - t0)
            ms.append(api.timing(TIMER_DVR_POWER)[0])
        flops, products = power_flops(ld, steps)
        t_power = float(np.median(ms)) * 1e-3
        print(json.dumps(dict(figure="power", dim=dim, ld=ld, n_steps=steps, halvings=s["halvings"], products=products, power_ms=1e3 * t_power,
                              call_s=float(np.median(wall)), tflop=flops / 1e12, tflops=flops / t_power / 1e12, fraction_of_fp64_mfma_peak=flops / t_power / PEAK)), flush=True)
        # one application per output
        api.dvr_apply(2, n, U, psi0, 1)
        t0 = time.perf_counter()
        psi = api.dvr_apply(2, n, U, psi0, 26)
        t_apply = (time.perf_counter() - t0) / 26
        print(json.dumps(dict(figure="apply", s_per_application=t_apply, gbytes_per_application=16.0 * dim * dim / 1e9,
                              norm_after_26_outputs=float(np.vdot(psi[-1], psi[-1]).real * dx))), flush=True)
        # the yardstick: stepping with the one-step propagator, 4096 applications per call
        U1 = api.dvr_propagator(2, n, H, W, s["dt"], 1, device_out=True)
        api.dvr_apply(2, n, U1, psi0, 8)
        t0 = time.perf_counter()
        done, v = 0, psi0
        while done < steps:
            T = min(4096, steps - done)
            v = api.dvr_apply(2, n, U1, v, T)[-1]
            done += T
        t_step = time.perf_counter() - t0
        outputs = s["total_step"] // steps + 1
        print(json.dumps(dict(figure="stepping", steps_per_output=steps, s_per_output=t_step, s_per_step=t_step / steps, outputs_of_a_full_run=outputs,
                              stepping_s_full_run=t_step * (outputs - 1), powers_s_full_run=float(np.median(wall)) + t_apply * (outputs - 1),
                              difference_from_power=float(np.linalg.norm(v - psi[0]) / np.linalg.norm(psi0)))), flush=True)
        # what is in the interior once the packet has left: the absorbing box [-6, 6] against a reflective box [-10, 22] whose wall the packet
        # has not reached by then
        small = dict(xmin=-6.0, xmax=6.0, x0=-3.0, output_time=s["output_time"])
        sa = exact.setup(ln_e, boundary=exact.ABSORBING, **small)
        Ha, _, Ba = api.dvr_hamiltonian(2, exact.DAC, exact.REFLECTIVE, sa["x"][0], sa["dx"], sa["n_grids"], mass)
        Wa = api.dvr_absorber(sa["x"][0], sa["dx"], sa["n_grids"], mass, sa["xmin"], sa["xmax"], sa["absorbing_length"])
        Ua = api.dvr_propagator(2, sa["n_grids"], Ha, Wa, sa["dt"], sa["output_step"], device_out=True)
        pa = exact.to_diabatic(exact.initial_adiabatic_psi(sa["x"], sa["x0"], sa["p0"], sa["sigma_x"], 2), Ba)
        k_out = int(1.5 * (sa["xmax"] - sa["x0"]) / (sa["p0"] / mass) / sa["output_time"]) + 1
        absorbed = api.dvr_apply(2, sa["n_grids"], Ua, pa, k_out)
        sr = exact.setup(ln_e, boundary=exact.REFLECTIVE, xmin=-10.0, xmax=22.0, x0=-3.0, output_time=s["output_time"])
        Hr, _, Br = api.dvr_hamiltonian(2, exact.DAC, exact.REFLECTIVE, sr["x"][0], sr["dx"], sr["n_grids"], mass)
        lam, V = np.linalg.eigh(Hr)
        pr = exact.to_diabatic(exact.initial_adiabatic_psi(sr["x"], sr["x0"], sr["p0"], sr["sigma_x"], 2), Br)
        free = api.dvr_propagate(2, sr["n_grids"], V, lam, pr, np.array([k_out * sa["output_time"]]))[0]
        inside_a = (sa["x"] >= -6.0) & (sa["x"] <= 6.0)
        inside_r = (sr["x"] >= -6.0) & (sr["x"] <= 6.0)
        pop = lambda v, m, d: float(sum(np.vdot(u[m], u[m]).real for u in v.reshape(2, -1)) * d)
        print(json.dumps(dict(figure="return", box=[-6.0, 6.0], dx=sa["dx"], t=k_out * sa["output_time"], interior_population_absorbing=pop(absorbed[-1], inside_a, sa["dx"]),
                              interior_population_open_box=pop(free, inside_r, sr["dx"]))), flush=True)
    finally:
        api.close()
    if "--no-e2e" not in args:
        with tempfile.TemporaryDirectory() as out:
            t0 = time.perf_counter()
            try:
                r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "exact_dvr.py"), "%g" % ln_e, out, "text", "absorbing"], capture_output=True, text=True,
                                   timeout=e2e_limit)
                size = sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out))
                print(json.dumps(dict(figure="e2e", seconds=time.perf_counter() - t0, returncode=r.returncode, output_gbytes=size / 1e9,
                                      tail=r.stdout.strip().splitlines()[-4:])), flush=True)
            except subprocess.TimeoutExpired:
                print(json.dumps(dict(figure="e2e", seconds=None, note="not finished within %d s" % e2e_limit)), flush=True)


if __name__ == "__main__":
    main()
