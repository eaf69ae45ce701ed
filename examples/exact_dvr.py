"""Exact DVR dynamics of Tully's dual avoided crossing at the defaults of the reference's schrodinger_equation/input.py (mass 2000,
x0 = -8, box [-15, 15], dx <= 0.1, sigma_p = p0 / 20, about 50 outputs): the six files of schrodinger_equation/main.cpp in an output
directory and the final stdout line.  Run on a GPU box:
    python examples/exact_dvr.py [lnE] [out_dir] [text|npy|none] [reflective|periodic|absorbing] [flux] [spectrum]
With `absorbing` the packet leaves the box through an absorbing region on either side (no eigh).  `absorbing flux` runs until
all of it has left and accounts for it: absorbed.txt, and a last line with the head of the final line, the absorbed population on the left
(reflection) and on the right (transmission) per adiabatic surface, and what is left in the box.  `absorbing flux spectrum` resolves that in
energy from the same packet: spectrum.txt (64 energies over p0 +- 3 sigma_p), and per energy the fractions of the channels."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import gaussian_process_liouville_equation_amd as pkg  # noqa: E402
from gaussian_process_liouville_equation_amd import exact  # noqa: E402

ln_e = float(sys.argv[1]) if len(sys.argv) > 1 else 0.0
out_dir = sys.argv[2] if len(sys.argv) > 2 else "exact_dvr_out"
write_phase = sys.argv[3] if len(sys.argv) > 3 else "text"
boundary = {"reflective": exact.REFLECTIVE, "absorbing": exact.ABSORBING}.get(sys.argv[4] if len(sys.argv) > 4 else "", exact.PERIODIC)
flux = len(sys.argv) > 5 and sys.argv[5] == "flux"
spectrum = flux and len(sys.argv) > 6 and sys.argv[6] == "spectrum"
api = pkg.open_api(0)
try:
    res = exact.run(api, model=exact.DAC, num_pes=2, boundary=boundary, ln_energy=ln_e, out_dir=out_dir,
                    write_phase=None if write_phase == "none" else write_phase, log=print, **(dict(flux=True, until_absorbed=True) if flux else {}), **(dict(spectrum=64) if spectrum else {}))
    s = res["setup"]
    timing = f"propagator {res['propagator_seconds']:.2f} s" if boundary == exact.ABSORBING else f"eigh {res['eigh_seconds']:.2f} s"
    print(f"grid: {s['n_grids']} points, dx = {s['dx']:g}; {timing}; {len(res['records'])} outputs, "
          f"{1e3 * res['seconds_per_output']:.1f} ms per output step; total {res['total_seconds']:.1f} s")
    print("final populations:", np.array2string(res["records"][-1]["populations"], precision=6))
    print(res["final_line"])
    if flux:
        print(res["scattering_line"])
    if spectrum:
        # per energy: E, then reflection and transmission per surface as fractions of what the absorber took at that energy (a weak channel's
        # figure may be slightly negative); energies the packet hardly holds are left out
        rho = res["spectrum"][:, 1:]
        held = rho.sum(axis=1) > 1e-3 * rho.sum(axis=1).max()
        print(f"spectrum over 2^{res['spectrum_levels']} steps, {res['spectrum_seconds']:.2f} s; left in the box after them: {res['spectrum_remaining']:.3g}")
        for row in res["spectrum"][held]:
            print(" ".join("%g" % v for v in [row[0], *(row[1:] / row[1:].sum())]))
finally:
    api.close()
