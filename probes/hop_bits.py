"""SHA-256 digests of every output array of every gple_hop_* entry point, for comparing two builds of the library bit for bit: the tests compare the
hop kernels with numpy inside tolerances, which a changed FMA contraction passes.  Run it once per build, each in a process of its own, and compare
the two files byte for byte (probes/README.md):

    python probes/hop_bits.py --lib probes/ab/libA.so --out out/hop_bits_A.json
    python probes/hop_bits.py --lib probes/ab/libB.so --out out/hop_bits_B.json
    cmp out/hop_bits_A.json out/hop_bits_B.json

The cases are the case tables of the tests (tests/test_gpu_hop.py, _mf, _sqc, _deco, tests/hop_mash_cases.py: model, levels, p0, dt,
steps, start surface, built-in or tabulated at dx = 1 / 16) with the tests' packet (x0 = -4, sigma_p = p0 / 20, sigma_x = 1 / (2 sigma_p)), bounds
+-6 and mass 2000, on 300 trajectories (a tail that is no multiple of 64 or of 256); the grouped calls take 3 groups of 100 with the packets p0,
0.9 p0 and 1.1 p0 (the last with sigma_x = 0: the select of the centre) and the time steps dt, dt, dt / 2.  Per case: sample, evolve and observe,
plain and grouped, for fewest switches (with each of the four decoherence modes), Ehrenfest, SQC (both windows) and MASH, and hop_bin /
hop_density of the fewest-switches end state; one case more goes through device tensors.  Beside the digests the file holds, per fewest-switches
and MASH case, the hops taken, the frustrated hops and the finished trajectories, so that a reader sees the branches were taken.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gaussian_process_liouville_equation_amd as pkg  # noqa: E402
from gaussian_process_liouville_equation_amd import pes  # noqa: E402
from tests import hop_mash_cases, test_gpu_hop, test_gpu_hop_deco, test_gpu_hop_mf, test_gpu_hop_sqc  # noqa: E402
from tests import hop_numpy as HN  # noqa: E402

N, GROUPS, PER = 300, 3, 100
X0, MASS, LEFT, RIGHT, SEED = -4.0, 2000.0, -6.0, 6.0, 20250117
MODES = (None, "edc", "collapse_hop", "collapse_attempt")
GRID = (LEFT, (RIGHT - LEFT) / 15, 16, 0.0, 4.0, 9)


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def packet(p0):
    return X0, p0, 1.0 / (2.0 * p0 / 20.0), p0 / 20.0


def group_tables(c):
    packets = np.array([packet(c["p0"]), packet(0.9 * c["p0"]), packet(1.1 * c["p0"])])
    packets[2, 2] = 0.0
    return packets, np.array([c["dt"], c["dt"], c["dt"] / 2.0])


class Models:
    """the model id of a case on the context: a table is defined once per (model, levels)"""

    def __init__(self, api):
        self.api, self.ids = api, {}

    def __call__(self, c):
        if not c.get("tabulated"):
            return c["model"]
        key = (c["model"], c["N"])
        if key not in self.ids:
            self.ids[key] = self.api.pes_define(c["N"], *pes.tabulate(HN.scalar_function(HN.builtin(*key)), -8.0, 1.0 / 16.0, 257))
        return self.ids[key]

    def close(self):
        for model in self.ids.values():
            self.api.pes_undefine(model)


def fewest_switches(api, model, c, out, counts, device=False):
    n_pes, s0, reverse = c["N"], c.get("surface0", 0), c.get("reverse", False)
    packets, dts = group_tables(c)
    start = api.hop_sample(n_pes, model, N, SEED, *packet(c["p0"]), s0, trajectory_offset=5, device_out=device)
    gstart = api.hop_sample_groups(n_pes, model, PER, SEED, packets, s0, trajectory_offset=5, device_out=device)
    out["sample"], out["sample_groups"] = digest(*start), digest(*gstart)
    for mode in MODES:
        name = mode or "none"
        copy = tuple(a.clone() for a in start) if device else start
        end = api.hop_evolve(n_pes, model, copy, SEED, MASS, c["dt"], 0, c["steps"], LEFT, RIGHT, reverse=reverse, trajectory_offset=5, decoherence=mode)
        hops = np.zeros((N, 2), dtype=np.int32)
        gcopy = gstart
        if device:
            import torch
            gcopy, hops = tuple(a.clone() for a in gstart), torch.zeros((N, 2), dtype=torch.int32, device=start[0].device)
        gend, hops = api.hop_evolve_groups(n_pes, model, gcopy, PER, SEED, MASS, dts, 0, c["steps"], LEFT, RIGHT, reverse=reverse, trajectory_offset=5, hops=hops,
                                           decoherence=mode)
        api.synchronize()
        out[f"evolve_{name}"], out[f"evolve_groups_{name}"], out[f"hops_{name}"] = digest(*end), digest(*gend), digest(hops)
        out[f"observe_{name}"] = digest(api.hop_observe(n_pes, model, end, MASS))
        out[f"observe_groups_{name}"] = digest(api.hop_observe_groups(n_pes, model, gend, PER, MASS))
        hops, status = (a.cpu().numpy() if device else a for a in (hops, gend[4]))
        counts[name] = dict(taken=int(hops[:, 0].sum()), frustrated=int(hops[:, 1].sum()), finished=int((status != 0).sum()))
        if mode is None:
            acc = api.hop_bin(n_pes, model, end, GRID, bin_all=True)
            out["bin"] = digest(acc)
            more = api.hop_bin(n_pes, model, gend, GRID, acc=acc)  # GPLE_HOP_ACCUMULATE; a device acc is added to in place
            out["bin_accumulate"] = digest(more)
            out["density"] = digest(api.hop_density(n_pes, GRID, more, 2 * N))
            api.synchronize()


def mean_field(api, model, c, out):
    n_pes, s0 = c["N"], c.get("surface0", 0)
    packets, dts = group_tables(c)
    start = api.hop_sample(n_pes, model, N, SEED, *packet(c["p0"]), s0)
    gstart = api.hop_sample_groups(n_pes, model, PER, SEED, packets, s0)
    end = api.hop_evolve_mf(n_pes, model, start, MASS, c["dt"], c["steps"], LEFT, RIGHT)
    gend = api.hop_evolve_groups_mf(n_pes, model, gstart, PER, MASS, dts, c["steps"], LEFT, RIGHT)
    out["evolve"], out["evolve_groups"] = digest(*end), digest(*gend)
    out["observe"] = digest(api.hop_observe_mf(n_pes, model, end, MASS))
    out["observe_groups"] = digest(api.hop_observe_groups_mf(n_pes, model, gend, PER, MASS))
    out["finished"] = int((gend[4] != 0).sum())


def sqc(api, model, c, window, out):
    n_pes, s0 = c["N"], c.get("surface0", 0)
    packets, dts = group_tables(c)
    gamma = (np.sqrt(3.0) - 1.0) / 2.0 if window == "square" else 1.0 / 3.0
    start = api.hop_sample_sqc(n_pes, model, N, SEED, *packet(c["p0"]), s0, window=window, trajectory_offset=5)
    gstart = api.hop_sample_groups_sqc(n_pes, model, PER, SEED, packets, s0, window=window, trajectory_offset=5)
    out["sample"], out["sample_groups"] = digest(*start), digest(*gstart)
    end = api.hop_evolve_sqc(n_pes, model, start, MASS, c["dt"], c["steps"], LEFT, RIGHT, gamma)
    gend = api.hop_evolve_groups_sqc(n_pes, model, gstart, PER, MASS, dts, c["steps"], LEFT, RIGHT, gamma)
    out["evolve"], out["evolve_groups"] = digest(*end), digest(*gend)
    out["observe"] = digest(api.hop_observe_sqc(n_pes, model, end, MASS, window=window))
    out["observe_groups"] = digest(api.hop_observe_groups_sqc(n_pes, model, gend, PER, MASS, window=window))
    out["finished"] = int((gend[4] != 0).sum())


def mash(api, model, c, out, counts):
    s0 = c.get("surface0", 0)
    packets, dts = group_tables(c)
    start = api.hop_sample_mash(2, model, N, SEED, *packet(c["p0"]), s0, trajectory_offset=5)
    gstart = api.hop_sample_groups_mash(2, model, PER, SEED, packets, s0, trajectory_offset=5)
    out["sample"], out["sample_groups"] = digest(*start), digest(*gstart)
    end = api.hop_evolve_mash(2, model, start, MASS, c["dt"], c["steps"], LEFT, RIGHT)
    gend, hops = api.hop_evolve_groups_mash(2, model, gstart, PER, MASS, dts, c["steps"], LEFT, RIGHT, hops=np.zeros((N, 2), dtype=np.int32))
    out["evolve"], out["evolve_groups"], out["hops"] = digest(*end), digest(*gend), digest(hops)
    out["observe"] = digest(api.hop_observe(2, model, end, MASS))
    out["observe_groups"] = digest(api.hop_observe_groups(2, model, gend, PER, MASS))
    counts.update(taken=int(hops[:, 0].sum()), frustrated=int(hops[:, 1].sum()), finished=int((gend[4] != 0).sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="the build of libgple_hip.so to load (default: the tree's)")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    if a.lib:
        pkg.LIB_PATH = os.path.abspath(a.lib)
    api = pkg.open_api(0)
    models = Models(api)
    digests, counts = {}, {}
    try:
        hop_cases = test_gpu_hop.CASES
        assert all(base in hop_cases for base, _ in test_gpu_hop_deco.CASES.values())  # the decoherence cases are these, with a mode each
        for name, c in hop_cases.items():
            digests[f"fssh/{name}"], counts[f"fssh/{name}"] = {}, {}
            fewest_switches(api, models(c), c, digests[f"fssh/{name}"], counts[f"fssh/{name}"])
        digests["fssh/dac10/device"], counts["fssh/dac10/device"] = {}, {}
        fewest_switches(api, hop_cases["dac10"]["model"], hop_cases["dac10"], digests["fssh/dac10/device"], counts["fssh/dac10/device"], device=True)
        for name, c in test_gpu_hop_mf.CASES.items():
            digests[f"mf/{name}"] = {}
            mean_field(api, models(c), c, digests[f"mf/{name}"])
        for name, c in test_gpu_hop_sqc.CASES.items():
            for window in test_gpu_hop_sqc.WINDOWS:
                digests[f"sqc/{name}/{window}"] = {}
                sqc(api, models(c), c, window, digests[f"sqc/{name}/{window}"])
        for name, c in hop_mash_cases.CASES.items():
            c = {"N": 2, **c}
            digests[f"mash/{name}"], counts[f"mash/{name}"] = {}, {}
            mash(api, models(c), c, digests[f"mash/{name}"], counts[f"mash/{name}"])
        models.close()
    finally:
        api.close()
    taken = sum(m["taken"] for k, v in counts.items() for m in (v.values() if k.startswith("fssh/") else [v]))
    with open(a.out, "w") as f:
        json.dump(dict(probe="hop_bits", trajectories=N, groups=[GROUPS, PER], counts=counts, digests=digests), f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(dict(probe="hop_bits", out=a.out, cases=len(digests), arrays=sum(len(v) for v in digests.values()), hops_taken=taken)))


if __name__ == "__main__":
    main()
