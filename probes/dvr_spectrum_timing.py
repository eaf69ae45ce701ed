"""Timing and figures of the energy-resolved spectrum of one absorbing DVR run (gple_dvr_spectrum, csrc/gple_dvr_spectrum.hip) at
the ln E = 0 defaults of schrodinger_equation/input.py (n = 1935, dim 3870) with 64 energies.  One JSON line per figure:
  spectrum  GPLE_TIMER_DVR_SPECTRUM of one gple_dvr_spectrum call (median of --reps after a warm-up) and the whole call; by count the real-GEMM
            flops of the squarings (lower tiles) and of the thin products, with the rate against the 78.6 TFLOP/s fp64 MFMA peak;
            GPLE_TIMER_DVR_POWER of gple_dvr_propagator (output_step steps) in the same process beside it; the work space
  run       exact.run(absorbing, flux, until_absorbed, spectrum=64) without phase.txt: the scattering line, and the fractions of the channels at the
            two energies next to E(p0) from spectrum.txt
  packets   two packets of p0 -+ sigma_p / 2 on the same grid, H, W and energies: the largest difference of their channel fractions where both
            densities exceed a tenth of their peaks
    python probes/dvr_spectrum_timing.py [--reps 3] [--levels 17] [--no-run] [--ln-e 0]"""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gaussian_process_liouville_equation_amd as pkg  # noqa: E402
from gaussian_process_liouville_equation_amd import exact  # noqa: E402

PEAK = 78.6e12
TIMER_DVR_POWER, TIMER_DVR_SPECTRUM = 9, 11
N_E = 64


def flops(ld, levels, nep, channels, tile=64):
    """(squarings and P4, thin products): real-GEMM flops by count.  A lower-tile product computes nt (nt + 1) / 2 tiles of ld^3 / nt^2 each"""
    nt = ld // tile
    lower = 2.0 * tile * tile * ld * (nt * (nt + 1) // 2)
    thin = 4 * 2.0 * ld * ld * (levels * nep + 64 + (1 + channels) * nep)  # per level, what is left, P X
    return (6 + 4 * levels) * lower, thin


def main():
    args = sys.argv[1:]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 3
    ln_e = float(args[args.index("--ln-e") + 1]) if "--ln-e" in args else 0.0
    levels = int(args[args.index("--levels") + 1]) if "--levels" in args else 17  # 2^17 / 64 = 2048 >= 1860, where the default run stops
    s = exact.setup(ln_e, boundary=exact.ABSORBING)
    n, dx, x, mass = s["n_grids"], s["dx"], s["x"], s["mass"]
    dim, ld = 2 * n, (2 * n + 63) // 64 * 64
    n_left = int(np.sum(x < (s["xmin"] + s["xmax"]) / 2.0))
    api = pkg.open_api(0)
    api.enable_timing(True)
    try:
        H, E_ad, B = api.dvr_hamiltonian(2, exact.DAC, exact.REFLECTIVE, x[0], dx, n, mass)
        W = api.dvr_absorber(x[0], dx, n, mass, s["xmin"], s["xmax"], s["absorbing_length"])
        psi0 = exact.to_diabatic(exact.initial_adiabatic_psi(x, s["x0"], s["p0"], s["sigma_x"], 2), B)
        E = exact.spectrum_energies(s, E_ad, N_E)
        power_ms = []
        for k in range(reps + 1):  # the first is the warm-up
            api.dvr_propagator(2, n, H, W, s["dt"], s["output_step"], device_out=True)
            power_ms.append(api.timing(TIMER_DVR_POWER)[0])
        ms, wall = [], []
        for k in range(reps + 1):
            t0 = time.perf_counter()
            rho, _, left = api.dvr_spectrum(2, n, H, W, s["dt"], levels, B, n_left, psi0, E)
            wall.append(time.perf_counter() - t0)
            ms.append(api.timing(TIMER_DVR_SPECTRUM)[0])
        f_square, f_thin = flops(ld, levels, N_E, 4)
        t_spec, t_power = float(np.median(ms[1:])) * 1e-3, float(np.median(power_ms[1:])) * 1e-3
        print(json.dumps(dict(figure="spectrum", dim=dim, ld=ld, n_E=N_E, levels=levels, dt=s["dt"], spectrum_ms=1e3 * t_spec, call_s=float(np.median(wall[1:])),
                              power_ms=1e3 * t_power, power_steps=s["output_step"], squarings_tflop=f_square / 1e12, thin_tflop=f_thin / 1e12,
                              thin_over_squarings=f_thin / f_square, tflops=(f_square + f_thin) / t_spec / 1e12,
                              fraction_of_fp64_mfma_peak=(f_square + f_thin) / t_spec / PEAK, work_gbytes=8.0 * (7 * ld * ld + ld + 22 * ld * N_E) / 1e9,
                              remaining=left * dx)), flush=True)
        if "--no-run" not in args:
            with tempfile.TemporaryDirectory() as out:
                t0 = time.perf_counter()
                res = exact.run(api, model=exact.DAC, num_pes=2, boundary=exact.ABSORBING, ln_energy=ln_e, out_dir=out, write_phase=None, flux=True,
                                until_absorbed=True, spectrum=N_E)
                rows = np.array([[float(v) for v in line.split()] for line in open(os.path.join(out, "spectrum.txt")).read().splitlines()])
            mid = rows[N_E // 2 - 1:N_E // 2 + 1]
            print(json.dumps(dict(figure="run", seconds=time.perf_counter() - t0, stop_time=res["stop_time"], scattering_line=res["scattering_line"],
                                  spectrum_levels=res["spectrum_levels"], spectrum_seconds=res["spectrum_seconds"], spectrum_remaining=res["spectrum_remaining"],
                                  energy_of_p0=float(exact.spectrum_energies(s, E_ad, 1)[0]), energies=mid[:, 0].tolist(),
                                  fractions=(mid[:, 1:] / mid[:, 1:].sum(axis=1, keepdims=True)).tolist(), most_negative_rho=float(rows[:, 1:].min()),
                                  largest_rho=float(rows[:, 1:].max()))), flush=True)
        a = []
        for sign in (-0.5, 0.5):
            packet = exact.to_diabatic(exact.initial_adiabatic_psi(x, s["x0"], s["p0"] + sign * s["sigma_p"], s["sigma_x"], 2), B)
            a.append(api.dvr_spectrum(2, n, H, W, s["dt"], levels, B, n_left, packet, E, want_remaining=False)[0].reshape(N_E, 4))
        total = [v.sum(axis=1) for v in a]
        both = (total[0] > 0.1 * total[0].max()) & (total[1] > 0.1 * total[1].max())
        frac = [v[both] / t[both, None] for v, t in zip(a, total)]
        print(json.dumps(dict(figure="packets", p0=[s["p0"] - 0.5 * s["sigma_p"], s["p0"] + 0.5 * s["sigma_p"]], energies_compared=int(both.sum()),
                              largest_fraction_difference=float(np.abs(frac[0] - frac[1]).max()),
                              largest_difference_per_channel=np.abs(frac[0] - frac[1]).max(axis=0).tolist())), flush=True)
    finally:
        api.close()


if __name__ == "__main__":
    main()
