"""CPU: csrc/gple_g6.h, the one source of the "%g" conversion that the device kernels compile too, against the C library's snprintf("%g") on
finite doubles.  tests/cpp/g6_check.cpp is a stand-alone host program: random bit patterns, every power of two, every decade
boundary and carry, and the seven-digit strings around every tie of the six-digit rounding, each with both neighbours and its negative."""
import os
import re
import subprocess

from tests.conftest import ROOT

RANDOM_COUNT = 20_000_000  # random 64-bit patterns (splitmix64, seeded)
TIE_STRIDE = 4             # every 4th six-digit prefix of the tie strings and both ends (1, the whole enumeration, takes about twice as long)


def test_header_matches_snprintf(tmp_path):
    exe = str(tmp_path / "g6_check")
    subprocess.run(["g++", "-O2", "-std=c++20", "-Wall", "-Wextra", "-pthread", os.path.join(ROOT, "tests", "cpp", "g6_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe, str(RANDOM_COUNT), str(TIE_STRIDE)], capture_output=True, text=True)
    print(run.stdout)
    found = re.search(r"compared (\d+) values, (\d+) mismatches", run.stdout)
    assert found, run.stdout + run.stderr
    assert int(found.group(1)) > 1.9 * RANDOM_COUNT  # each pattern and its negative, but for the non-finite ones
    assert int(found.group(2)) == 0 and run.returncode == 0, run.stdout


def test_kernels_emulated_on_host_threads(tmp_path):
    """csrc/gple_format.hip compiled for the host (tests/cpp/format_emulation.cpp: a host thread per work-item, barriers for __syncthreads): the
    layout, both scans, the 64-bit offsets and the staging at the destination's alignment give snprintf's bytes and touch nothing else"""
    exe = str(tmp_path / "format_emulation")
    subprocess.run(["g++", "-O1", "-std=c++20", "-pthread", "-I/opt/rocm/include", "-x", "c++", os.path.join(ROOT, "tests", "cpp", "format_emulation.cpp"), "-o", exe,
                    "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "emulation done, 0 bad" in run.stdout, run.stdout + run.stderr
