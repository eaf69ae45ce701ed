"""CPU: csrc/gple_d2.h, the one source of the text-to-double conversion that the device kernels compile too, against the C library's strtod;
csrc/gple_parse.hip emulated on host threads; and the host pieces of reconstruct.run_files with a stub api."""
import os
import re
import subprocess

import numpy as np
import pytest

from gaussian_process_liouville_equation_amd import _capi, reconstruct as R
from tests.conftest import ROOT
from tests.test_recon_cross_host import RecordingApi

RANDOM_COUNT = 10_000_000  # random 64-bit patterns (splitmix64, seeded), four texts each and their negatives


def test_header_matches_strtod(tmp_path):
    exe = str(tmp_path / "d2_check")
    subprocess.run(["g++", "-O2", "-std=c++20", "-Wall", "-Wextra", "-pthread", os.path.join(ROOT, "tests", "cpp", "d2_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe, str(RANDOM_COUNT)], capture_output=True, text=True)
    print(run.stdout)
    found = re.search(r"compared (\d+) values, (\d+) mismatches", run.stdout)
    assert found, run.stdout + run.stderr
    assert int(found.group(1)) > 8 * RANDOM_COUNT
    assert int(found.group(2)) == 0 and run.returncode == 0, run.stdout


def test_kernels_emulated_on_host_threads(tmp_path):
    """csrc/gple_parse.hip compiled for the host (tests/cpp/parse_emulation.cpp: a host thread per work-item): chunk boundaries at every alignment
    of the text pointer, tokens across them, the line count, both scans and the compaction give strtod's values and touch nothing else"""
    exe = str(tmp_path / "parse_emulation")
    subprocess.run(["g++", "-O1", "-std=c++20", "-pthread", "-I/opt/rocm/include", "-x", "c++", os.path.join(ROOT, "tests", "cpp", "parse_emulation.cpp"), "-o", exe,
                    "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and re.search(r"emulation done, \d+ cases, 0 bad", run.stdout), run.stdout + run.stderr


def test_read_grid(tmp_path):
    path = tmp_path / "x.txt"
    path.write_text("-1.5\n0\n 2.5e-3  7\n\n1e+300")
    assert np.array_equal(R.read_grid(path), [-1.5, 0.0, 2.5e-3, 7.0, 1e300])
    path.write_text("")
    assert R.read_grid(path).shape == (0,)


def block_text(k, nx=2, np_=3, nq=4):
    """output k of a hand-written phase.txt: re = k + q / 4 + j / 32 (six digits at most), im = -j for cell j of plane q"""
    return "".join("".join(f" {k + q / 4 + j / 32:g} {-j:g}" for j in range(nx * np_)) + "\n" for q in range(nq)) + "\n"


def test_phase_blocks(tmp_path):
    path = tmp_path / "phase.txt"
    texts = [block_text(k) for k in range(3)]
    path.write_text("".join(texts))
    assert [bytes(b).decode() for b in R.phase_blocks(path, 2, 2, 3)] == texts
    assert [bytes(b).decode() for b in R.phase_blocks(path, 2, 2, 3, outputs=[2])] == texts[2:]
    assert [bytes(b).decode() for b in R.phase_blocks(path, 2, 2, 3, outputs=[0, 2])] == [texts[0], texts[2]]
    assert list(R.phase_blocks(path, 2, 2, 3, outputs=[])) == []
    # stops behind the last output asked for: what follows is not looked at
    path.write_text(texts[0] + texts[1] + "garbage")
    assert [bytes(b).decode() for b in R.phase_blocks(path, 2, 2, 3, outputs=[1])] == texts[1:2]
    with pytest.raises(ValueError, match="output 2"):
        list(R.phase_blocks(path, 2, 2, 3))
    # a block cut short: a line missing, or the file ending inside it
    short = "".join(texts[1].split("\n", 1)[1:])
    path.write_text(texts[0] + short + texts[2])
    blocks = R.phase_blocks(path, 2, 2, 3)
    assert bytes(next(blocks)).decode() == texts[0]
    with pytest.raises(ValueError, match="output 1"):
        next(blocks)
    path.write_text(texts[0] + texts[1][:40])
    with pytest.raises(ValueError, match="output 1"):
        list(R.phase_blocks(path, 2, 2, 3))
    assert [bytes(b).decode() for b in R.phase_blocks(path, 2, 2, 3, outputs=[0])] == texts[:1]
    path.write_text("")
    assert list(R.phase_blocks(path, 2, 2, 3)) == []


class StateApi(RecordingApi):
    """RecordingApi whose survey depends on the state it is given, and which keeps the states"""

    def __init__(self, nx, np_):
        super().__init__(nx, np_)
        self.lib, self.states, self.seeds = None, [], []

    def grid_survey(self, num_pes, model, rho, x, p, mass, dx, dp):
        assert isinstance(rho, np.ndarray) and rho.dtype == np.complex128 and rho.shape == (2, 2, self.nx, self.np)
        self.states.append(rho.copy())
        s = super().grid_survey(num_pes, model, rho, x, p, mass, dx, dp)
        s[:, 0] = rho.real.max(axis=(2, 3)).ravel()
        s[[0, 3], 5] = [rho[0, 0].real.sum() * 1e-3, rho[1, 1].real.sum() * 1e-3]
        return s

    def grid_select(self, num_pes, rho, x, p, q, n, seed, uniform=False):
        self.seeds.append(seed)
        return super().grid_select(num_pes, rho, x, p, q, n, seed, uniform)


@pytest.fixture
def stub_searches(monkeypatch):
    monkeypatch.setattr(_capi, "minimize_neldermead", lambda lib, f, start, lower, upper, options=None: (list(np.clip(start, lower, upper)), f(list(start)), 1))
    monkeypatch.setattr(_capi, "minimize_auglag_eq", lambda lib, f, con, m, start, lower, upper, options=None: ([0.9 * v + 0.05 for v in start], f(list(start), True)[0], 1))


def test_run_files_host_route(tmp_path, stub_searches):
    nx, np_ = 2, 3
    x, p, t = np.array([-1.0, 1.0]), np.array([14.0, 15.0, 16.0]), np.array([0.0, 20.0, 40.0])
    run = tmp_path / "run"
    run.mkdir()
    for name, grid in (("x.txt", x), ("p.txt", p), ("t.txt", t)):
        (run / name).write_text("".join("%g\n" % v for v in grid))
    (run / "phase.txt").write_text("".join(block_text(k) for k in range(3)))
    states = [np.array([[k + q / 4 + j / 32 - 1j * j for j in range(nx * np_)] for q in range(4)]).reshape(2, 2, nx, np_) for k in range(3)]
    api = StateApi(nx, np_)
    recs = R.run_files(api, str(run), out_dir=str(tmp_path / "out"), model=1, n_points=6, seed=100, write_sim=True)
    assert len(recs) == 3 and [r["t"] for r in recs] == [0.0, 20.0, 40.0]
    assert api.seeds == [100] * 4 + [101] * 4 + [102] * 4
    # the same carry by hand: reconstruct() on the states built directly
    direct, hyper, energy = StateApi(nx, np_), None, None
    state = R.State(direct, 2, 1, x, p, 2000.0)
    for k, rho in enumerate(states):
        want = R.reconstruct(direct, state, rho, n_points=6, seed=100 + k, start=hyper, initial_energy=energy)
        hyper, energy = want["hyper"], want["initial_energy"]
        assert np.array_equal(api.states[k], rho)
        for key in ("hyper", "nlml", "factors", "sums_before", "sums_after", "initial_energy", "survey"):
            assert np.array_equal(recs[k][key], want[key]), key
    assert not np.array_equal(recs[0]["hyper"], recs[1]["hyper"]) and recs[2]["initial_energy"] == recs[0]["initial_energy"]
    # the files of run_mqcl
    out = tmp_path / "out"
    assert (out / "log.txt").read_text() == "".join(R.log_line(r["t"], r) for r in recs)
    assert (out / "choose.txt").read_text() == "".join(R.choose_block(r) for r in recs)
    assert len((out / "sim.txt").read_text().split("\n\n")) == 3 + 1 and "pred_after" not in recs[0]
    # outputs: one index alone starts afresh; the blocks before it are never read
    api = StateApi(nx, np_)
    one = R.run_files(api, str(run), model=1, n_points=6, seed=100, outputs=[2])
    assert len(one) == 1 and one[0]["index"] == 2 and one[0]["t"] == 40.0 and len(api.states) == 1 and api.seeds == [102] * 4
    fresh = R.reconstruct(direct, state, states[2], n_points=6, seed=102)
    assert np.array_equal(one[0]["hyper"], fresh["hyper"]) and one[0]["initial_energy"] == fresh["initial_energy"]
    # a block of another shape, an index beyond t.txt, a phase.txt shorter than t.txt
    (run / "p.txt").write_text("14\n16\n")
    with pytest.raises(ValueError, match="output 0"):
        R.run_files(StateApi(nx, 2), str(run), model=1, n_points=6)
    (run / "p.txt").write_text("14\n15\n16\n")
    with pytest.raises(ValueError):
        R.run_files(StateApi(nx, np_), str(run), model=1, n_points=6, outputs=[3])
    (run / "phase.txt").write_text(block_text(0) + block_text(1))
    with pytest.raises(ValueError, match="output 2"):
        R.run_files(StateApi(nx, np_), str(run), model=1, n_points=6)
