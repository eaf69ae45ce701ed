"""Cycle stamps inside rownormp_kernel (wave 0 of workgroup 0, one stamp behind the barrier that opens a step): barrier-to-barrier cycles of the twelve
steps of every diagonal 256-block (0 ... 7: the single steps D; 8 ... 11: the double steps (8, 9) ... (14, 15)) and of the last whole step in front of the
block, at C4r and C2.  Needs the instrumented build: `git apply probes/diag_stamps.patch && make -C gaussian_process_liouville_equation_amd/csrc` (one
LDS store and one s_memtime per stamped step, gple_debug_diag_stamps; revert afterwards).  The stamp costs a few scalar instructions and a wait for the
counter, and the whole steps are sensitive to exactly that: read the diagonal steps against each other and against their MFMA time, and take the
time of a whole step from the kernel time of an uninstrumented build.  Results: profiles/diag_steps.md."""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import gaussian_process_liouville_equation_amd as pkg
from gaussian_process_liouville_equation_amd import _capi as c
from tests.test_gpu_configs import config_inputs, THETA_R

tag = sys.argv[1] if len(sys.argv) > 1 else "build"
api = pkg.open_api(0)
get = api.lib.gple_debug_diag_stamps
get.argtypes = [ctypes.c_void_p]
for name, N, G in (("C4r", 4096, 512), ("C2", 1024, 256)):
    X, y, grid, _ = config_inputs(N, G, 1)
    fit = api.real_fit(THETA_R, X, y, 3)
    for rep in range(3):
        api.real_predict(fit, grid, flags=c.PREDICT_FULL)
    buf = np.zeros(2048, dtype=np.uint32)
    assert get(buf.ctypes.data_as(ctypes.c_void_p)) == 0
    n = int(buf[0])
    ids, t = buf[1:1 + 2 * n:2].astype(np.int64), buf[2:2 + 2 * n:2].astype(np.int64)
    d = (t[1:] - t[:-1]) % (1 << 32)
    per = {}
    for i in range(n - 1):
        a, b = ids[i], ids[i + 1]
        if a == 100 and b != 0:
            continue  # a stamped whole step that is not the last one in front of the diagonal block: the next stamp is many steps away
        if b == 200:
            continue  # the end of the unit: the epilogue is inside
        per.setdefault(int(a), []).append(int(d[i]))
    print(f"{tag} {name} kernel {api.last_contraction_kernel()} stamps {n} tiles {sum(1 for a in ids if a == 0)}")
    for k in sorted(per):
        v = np.array(per[k])
        print(f"{tag} {name} step {'whole' if k == 100 else k:>5} n {len(v):3d} median {int(np.median(v)):6d} min {v.min():6d} max {v.max():6d}")
    fit.release()
api.close()
