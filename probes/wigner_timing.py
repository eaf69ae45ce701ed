"""Timing of the Wigner transform (gple_wigner, csrc/gple_dvr.hip) at the grids of schrodinger_equation/input.py: n = 481 / 1921 / 3841
(ln E = -4 / 0 / 1), both boundaries, num_pes = 2, T = 1 and 8 output times per call.  Per case: device ms per output time from the
library's GPLE_TIMER_WIGNER events after a warm-up, the end-to-end time of the same call with host pointers, and the algorithmic rate
8 x (valid terms) x (computed elements) / time against the fp64 MFMA peak of 78.6 TFLOP/s.  Also the numpy restatement's time per output
at n = 481 (a CPU figure of this test helper, not of the reference).  One JSON line per case on stdout.
    python probes/wigner_timing.py [--quick] [--cases 3841:1:1,...]   (n:boundary:T)
    python probes/wigner_timing.py --eigh    numpy.linalg.eigh against torch.linalg.eigh on the GPU for the DAC Hamiltonian at dim 3842 / 7682"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gaussian_process_liouville_equation_amd as pkg  # noqa: E402
from gaussian_process_liouville_equation_amd import exact  # noqa: E402

PEAK = 78.6e12
GRIDS = {481: -4.0, 1921: 0.0, 3841: 1.0}


def valid_terms(n, n_p, boundary):
    a = np.arange(n)
    if boundary == exact.REFLECTIVE:
        return int(np.sum(2 * np.minimum(a, n - 1 - a) + 1)) * n_p
    return n * (2 * (n // 3) + 1) * n_p


def eigh_timing(api):
    import torch

    for ln_e in (0.0, 1.0):
        s = exact.setup(ln_e)
        H, _, _ = api.dvr_hamiltonian(2, exact.DAC, exact.PERIODIC, s["x"][0], s["dx"], s["n_grids"], s["mass"], want_states=False)
        t0 = time.perf_counter()
        w_np, _ = np.linalg.eigh(H)
        t_np = time.perf_counter() - t0
        Ht = torch.from_numpy(H).to("cuda")
        torch.linalg.eigh(Ht)  # warm-up (library load, workspace)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        w_t, _ = torch.linalg.eigh(Ht)
        torch.cuda.synchronize()
        t_t = time.perf_counter() - t0
        print(json.dumps(dict(dim=H.shape[0], numpy_eigh_s=t_np, torch_cuda_eigh_s=t_t, max_eigval_diff=float(np.abs(w_t.cpu().numpy() - w_np).max()),
                              omp_threads=os.environ.get("OMP_NUM_THREADS"))), flush=True)


def main():
    args = sys.argv[1:]
    if "--eigh" in args:
        api = pkg.open_api(0)
        eigh_timing(api)
        api.close()
        return
    quick = "--quick" in args
    cases = [(n, b, T) for n in GRIDS for b in (exact.PERIODIC, exact.REFLECTIVE) for T in (1, 8)]
    if "--cases" in args:
        cases = [tuple(int(v) for v in c.split(":")) for c in args[args.index("--cases") + 1].split(",")]
    api = pkg.open_api(0)
    api.enable_timing(True)
    reps = 2 if quick else 5
    for n, boundary, T in cases:
        s = exact.setup(GRIDS[n])
        x, p, dx = s["x"], s["p"], s["dx"]
        _, E, B = api.dvr_hamiltonian(2, exact.DAC, boundary, x[0], dx, n, s["mass"], want_h=False)
        psi1 = exact.to_diabatic(exact.initial_adiabatic_psi(x, s["x0"], s["p0"], s["sigma_x"], 2), B)
        psi = np.stack([np.roll(psi1, 7 * t) for t in range(T)])
        want_phase = T * 4 * n * len(p) * 16 <= (2 << 30)
        api.wigner(2, boundary, x[0], dx, p, psi, energies=E, mass=s["mass"], phase=want_phase, averages=True)  # warm-up
        dev, e2e = [], []
        for _ in range(reps):
            api.timing(4)
            t0 = time.perf_counter()
            api.wigner(2, boundary, x[0], dx, p, psi, energies=E, mass=s["mass"], phase=want_phase, averages=True)
            e2e.append(time.perf_counter() - t0)
            dev.append(api.timing(4)[0])
        ms = float(np.median(dev))
        flops = 8.0 * valid_terms(n, len(p), boundary) * 3 * T
        rec = dict(n_grids=n, boundary="periodic" if boundary == exact.PERIODIC else "reflective", num_pes=2, T=T,
                   kernel_ms_per_output=ms / T, kernel_ms_call=ms, e2e_ms_per_output=1e3 * float(np.median(e2e)) / T,
                   e2e_includes_phase_copy=want_phase, gflop_per_output=flops / T / 1e9, tflops=flops / (ms * 1e-3) / 1e12,
                   fraction_of_fp64_mfma_peak=flops / (ms * 1e-3) / PEAK)
        print(json.dumps(rec), flush=True)
    if not quick and "--cases" not in args:
        sys.path.insert(0, os.path.join(ROOT))
        from tests import dvr_numpy as DN
        s = exact.setup(-4.0)
        psi = exact.initial_adiabatic_psi(s["x"], s["x0"], s["p0"], s["sigma_x"], 2)
        t0 = time.perf_counter()
        DN.wigner(psi, 2, exact.PERIODIC, s["dx"], s["p"], dtype=np.complex128)
        print(json.dumps(dict(cpu_numpy_restatement_s_per_output=time.perf_counter() - t0, n_grids=481, boundary="periodic",
                              note="tests/dvr_numpy.py in complex128, all four elements; a CPU figure of the test helper, not the reference")))
    api.close()


if __name__ == "__main__":
    main()
