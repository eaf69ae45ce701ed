"""CPU: what `bench.py --dump-outputs DIR` writes — one float64 .npy per output, the complex grid outputs as (re, im) pairs per point, and
above the 64 MB budget one fixed, seeded sample of the grid points, the same for every array and every run."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _files(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_small_outputs_whole(tmp_path):
    M = 64
    out = torch.arange(5 * M, dtype=torch.float64).view(5, M)  # a complex element's (rows, M) buffer
    bench.dump_outputs(str(tmp_path), dict(bench.grid_outputs(out, True), fit_scalars=np.arange(4.0)), points=M)
    got = _files(tmp_path)
    assert sorted(got) == ["cutoff", "fit_scalars", "mean", "variance"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["mean"].shape == (M, 2) and got["mean"][3].tolist() == [6.0, 7.0]  # point 3: (re, im) = buffer[6], buffer[7]
    assert got["variance"][3] == 2 * M + 3 and got["cutoff"][3].tolist() == [3 * M + 6, 3 * M + 7]


def test_dump_samples_the_grid_above_the_budget(tmp_path):
    M = 1 << 20  # C5: six elements on a 1024 x 1024 grid, 192 MB in all
    arrays = {"element_scalars": np.ones((6, 2))}
    for e, cplx in enumerate([False, True, False, True, True, False]):
        out = torch.arange((5 if cplx else 3) * M, dtype=torch.float64).view(-1, M)
        arrays.update(bench.grid_outputs(out, cplx, prefix=f"element{e}_"))
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays, points=M)
    a, b = _files(tmp_path / "a"), _files(tmp_path / "b")
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 * 10**6
    assert all(np.array_equal(a[k], b[k]) for k in a)
    idx = a["sample_index"].astype(np.int64)
    assert len(idx) > M // 4 and np.all(np.diff(idx) > 0)
    assert a["element_scalars"].shape == (6, 2)
    assert np.array_equal(a["element1_mean"][:, 0], 2.0 * idx) and np.array_equal(a["element0_variance"], M + idx.astype(np.float64))
