"""numpy restatement of the grouped surface hopping calls (gple_hop_sample_groups / _evolve_groups / _observe_groups; include/gple.h, DESIGN.md §17,
"A curve in one launch") on top of tests/hop_numpy.py: every group is the plain call on its slice, with the group's offset, packet and time
step, plus what the grouped calls add: the zero-sigma rule of the sample and the hop counters of the evolve.

    sample_groups(), evolve_groups(), observe_groups()   the three entry points
    NumpyScanApi                                          the three Api methods (and the plain ones) on the restatement, for hopping.scan
"""
import numpy as np

from tests import hop_numpy as HN


def slices(n_groups, n_per_group):
    return [slice(g * n_per_group, (g + 1) * n_per_group) for g in range(n_groups)]


def sample_groups(potential, num_pes, n_per_group, seed, packets, surface0=0, trajectory_offset=0, dtype=np.float64):
    """gple_hop_sample_groups -> (x, p, b, surface, status): group g is hop_sample with the offset trajectory_offset + g n_per_group and the row
    (x0, p0, sigma_x, sigma_p) of packets; where a sigma is exactly 0 the coordinate is the centre exactly (a select), and b is the column of
    C at the x that results"""
    packets = np.asarray(packets, dtype=np.float64).reshape(-1, 4)
    ty = np.dtype(dtype).type
    parts = []
    for g, (x0, p0, sx, sp) in enumerate(packets):
        x, p, _, surface, status = HN.sample(potential, num_pes, n_per_group, seed, x0, p0, sx, sp, surface0, trajectory_offset + g * n_per_group, dtype)
        if sx == 0.0:
            x = np.full(n_per_group, ty(x0), dtype=dtype)
        if sp == 0.0:
            p = np.full(n_per_group, ty(p0), dtype=dtype)
        _, _, C, _ = HN.states(x, potential)
        parts.append((x, p, C[:, :, surface0].astype(HN.complex_of(dtype)), surface, status))
    return tuple(np.concatenate([part[q] for part in parts]) for q in range(5))


def evolve_groups(potential, state, n_per_group, seed, mass, dt, first_step, n_steps, x_left, x_right, reverse=False, trajectory_offset=0, hops=None):
    """gple_hop_evolve_groups on a copy -> (state, hops, diagnostics): group g is hop_evolve on its slice with dt[g]; hops (n, 2) int32 is a copy
    of the given counters (zeros for None) with the hops taken and the frustrated hops of the call added; the diagnostics are hop_numpy.evolve's,
    concatenated"""
    n = len(state[0])
    n_groups = n // n_per_group
    assert n_groups * n_per_group == n and len(dt) == n_groups
    hops = np.zeros((n, 2), dtype=np.int32) if hops is None else np.array(hops, dtype=np.int32)
    parts, diags, g = [], [], 0
    while g < n_groups:
        # neighbours with the same time step go through one plain call: trajectories are independent, so the bits are those of a call per group
        # (tests/test_hop_scan_host.py checks that), at a fraction of the interpreter's time
        last = g
        while last + 1 < n_groups and dt[last + 1] == dt[g]:
            last += 1
        sl = slice(g * n_per_group, (last + 1) * n_per_group)
        part, diag = HN.evolve(potential, tuple(a[sl] for a in state), seed, mass, dt[g], first_step, n_steps, x_left, x_right, reverse,
                               trajectory_offset + g * n_per_group)
        parts.append(part)
        diags.append(diag)
        hops[sl, 0] += diag["hops"].astype(np.int32)
        hops[sl, 1] += diag["frustrated"].astype(np.int32)
        g = last + 1
    out = tuple(np.concatenate([part[q] for part in parts]) for q in range(5))
    return out, hops, {key: np.concatenate([d[key] for d in diags]) for key in diags[0]}


def observe_groups(potential, state, n_per_group, mass):
    """gple_hop_observe_groups -> (n_groups, 4 N + 3): row g is hop_observe on the slice"""
    n_groups = len(state[0]) // n_per_group
    return np.stack([HN.observe(potential, tuple(a[sl] for a in state), mass) for sl in slices(n_groups, n_per_group)])


class NumpyScanApi(HN.NumpyHopApi):
    """Api.hop_sample_groups / hop_evolve_groups / hop_observe_groups on the restatement, beside the plain three of NumpyHopApi"""

    def hop_sample_groups(self, num_pes, model, n_per_group, seed, packets, surface0=0, trajectory_offset=0, device_out=False):
        self.calls.append(("sample_groups", len(packets), n_per_group))
        return sample_groups(self._potential(num_pes, model), num_pes, n_per_group, seed, packets, surface0, trajectory_offset, self.dtype)

    def hop_evolve_groups(self, num_pes, model, state, n_per_group, seed, mass, dt, first_step, n_steps, x_left, x_right, reverse=False, trajectory_offset=0,
                          hops=None):
        self.calls.append(("evolve_groups", first_step, n_steps))
        out, counted, _ = evolve_groups(self._potential(num_pes, model), state, n_per_group, seed, mass, dt, first_step, n_steps, x_left, x_right, reverse,
                                        trajectory_offset, hops)
        return out if hops is None else (out, counted)

    def hop_observe_groups(self, num_pes, model, state, n_per_group, mass):
        self.calls.append(("observe_groups",))
        return observe_groups(self._potential(num_pes, model), state, n_per_group, mass).astype(np.float64)
