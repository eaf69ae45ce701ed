"""GPU: gple_parse_g (text to doubles on the device) against Python's float(), bit for bit, its round trip with gple_format_g, and
reconstruct.run_files on directories the two exact solvers wrote.  Equality is bit for bit throughout: this feature has no tolerance."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
BAD_ARG = 1
TIMER_PARSE = 8
CHUNK = 4096  # bytes of text per workgroup (csrc/gple_kernels.h, PARSE_CHUNK)
KEYS = ("hyper", "nlml", "sums_before", "sums_after", "factors")


def _with_neighbours(v):
    v = np.asarray(v, dtype=np.float64)
    return np.concatenate([v, np.nextafter(v, np.inf), np.nextafter(v, -np.inf)])


@pytest.fixture(scope="module")
def pool():
    """the values of tests/test_gpu_format.py's pool: powers of two, decades, the ties of the six-digit rounding, specials, two random families"""
    parts = [_with_neighbours(np.ldexp(1.0, np.arange(-1074, 1024)))]
    parts.append(_with_neighbours([float(f"1e{k}") for k in range(-323, 309)] + [float(f"9.999995e{k}") for k in range(-323, 308)]))
    ties = [float(Fraction(10 * D + 5) * Fraction(10) ** k) for D in sorted(set(range(100000, 1000000, 997)) | {100000, 999999}) for k in range(-8, 9)]
    parts.append(_with_neighbours(ties))
    parts.append(np.array([0.0, math.inf, 5e-324, 2.2250738585072009e-308, 2.2250738585072014e-308, 1.7976931348623157e308, -1.23457e-308]))
    structured = np.concatenate(parts)
    rng = np.random.default_rng(20240607)
    bits = rng.integers(0, 2 ** 64, size=200_000, dtype=np.uint64).view(np.float64)
    scaled = rng.normal(size=200_000) * 10.0 ** rng.uniform(-20, 2, size=200_000)
    return np.concatenate([structured, -structured, [math.nan], bits, scaled])


def same_bits(got, want):
    """bit for bit, but any NaN equals any NaN (the library gives one quiet NaN; -0 is told from 0 by its sign bit)"""
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64))


@pytest.mark.parametrize("spec", ["%g", "%.17g"])
def test_values_match_python(gpu, pool, spec):
    tokens = [(spec % v).encode() for v in pool]
    got, lines = gpu.parse_g(b" ".join(tokens))
    want = np.array([float(t) for t in tokens])
    assert lines == 1 and same_bits(got, want)
    if spec == "%.17g":
        assert same_bits(got, pool)
        finite = np.isfinite(pool)
        assert np.array_equal(got[finite].view(np.uint64), pool[finite].view(np.uint64))


# (per_line, lines, lines_per_block): the issue's shapes; then, by this implementation's chunk of 4096 bytes, lines of 1.5 (" 1.5": four bytes a
# number) that are one number under a chunk, a chunk of numbers (the newline is the next chunk's first byte) and one number over, twice each
SHAPES = [(1, 5, 0), (7, 3, 1), (257, 3, 0), (4097, 17, 3)]
CHUNK_LINES = [CHUNK // 4 - 1, CHUNK // 4, CHUNK // 4 + 1]


@pytest.mark.parametrize("join", [False, True])
def test_round_trip_with_format_g(gpu, pool, join):
    """parse_g(format_g(v)) is float("%g" % v), and format_g of that gives the same bytes back — wherever "%g" itself does: for a few subnormals
    it does not, on any implementation ("%g" % 1.000004e-318 is 1e-318, whose nearest double prints as 9.99999e-319; the pool holds that value
    and its negative, twice each), so the second text is compared with Python's "%g" of the parsed values token by token, and with the first
    text as a whole whenever Python's own second text equals its first"""
    start = 0
    for per_line, lines, lines_per_block in SHAPES:
        v = pool[(start + np.arange(per_line * lines)) % len(pool)]
        start += 7919
        text = bytes(gpu.format_g(v, per_line, lines_per_block, join=join))
        got, got_lines = gpu.parse_g(text)
        assert got_lines == lines, (per_line, lines)
        assert same_bits(got, np.array([float("%g" % u) for u in v])), (per_line, lines)
        again = bytes(gpu.format_g(got, per_line, lines_per_block, join=join))
        python_again = [("%g" % float("%g" % u)).encode() for u in v]
        assert again.split() == python_again, (per_line, lines)
        assert (again == text) == (python_again == text.split()) and len(again.split(b"\n")) == len(text.split(b"\n")), (per_line, lines)
    for n in CHUNK_LINES:
        v = np.full(n, 1.5)
        text = bytes(gpu.format_g(v, n, 0, join=join))
        assert len(text) == 4 * n + 1 - join
        got, got_lines = gpu.parse_g(text + text)
        assert got_lines == 2 and same_bits(got, np.concatenate([v, v]))


def test_pointers_and_repeats(gpu, pool):
    import torch
    v = pool[(999 + np.arange(30000)) % len(pool)]
    text = bytes(gpu.format_g(v, 100, 7))
    want = np.array([float("%g" % u) for u in v])
    host, lines = gpu.parse_g(text)
    assert lines == 300 and same_bits(host, want)
    again, _ = gpu.parse_g(np.frombuffer(text, dtype=np.uint8))
    assert np.array_equal(host.view(np.uint64), again.view(np.uint64))
    out, lines_dev = gpu.parse_g(text, device_out=True)
    assert out.is_cuda and lines_dev == 300 and np.array_equal(out.cpu().numpy().view(np.uint64), host.view(np.uint64))
    for offset in (1, 7, 15):
        base = torch.zeros(offset + len(text), dtype=torch.uint8, device="cuda")
        assert base.data_ptr() % 16 == 0
        base[offset:] = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
        for _ in range(2):  # two calls: the same bits
            dev, dev_lines = gpu.parse_g(base[offset:])
            assert dev.is_cuda and dev_lines == 300
            assert np.array_equal(dev.cpu().numpy().view(np.uint64), host.view(np.uint64)), offset
    # count only equals the converting call's count; the timer counts calls
    f = gpu.lib.gple_parse_g
    count, lines_c = C.c_size_t(0), C.c_size_t(0)
    gpu.enable_timing(True)
    try:
        assert f(gpu.ctx, text, len(text), 0, None, 0, C.byref(count), C.byref(lines_c), None) == 0
        last, total, calls = gpu.timing(TIMER_PARSE)
        assert calls == 1 and last > 0 and total >= last
    finally:
        gpu.enable_timing(False)
    assert count.value == 30000 and lines_c.value == 300
    for blank in (b"", b" \n\t\r\n  "):
        values, n = gpu.parse_g(blank)
        assert len(values) == 0 and n == 0
    values, n = gpu.parse_g(b"", device_out=True)
    assert values.is_cuda and len(values) == 0 and n == 0


def test_errors(gpu):
    f = gpu.lib.gple_parse_g
    filler = (b" 1.5" * 15 + b"\n") * 200  # 61 bytes a line, 12200 bytes: three chunks
    last_start = (len(filler) // CHUNK) * CHUNK

    def with_token(text, where, token):
        return text[:where] + b" " + token + b" " + text[where + len(token) + 2:]

    for where, token in ((100, b"1x5"), (CHUNK - 3, b"12.5e+"), (last_start + 50, b"0x1p3"), (300, b"-"), (CHUNK + 9, b"1e"), (40, b"1" * 65),
                         (2 * CHUNK - 30, b"1" * 65), (77, b"12345678901234567891")):
        bad = with_token(filler, where, token)
        assert len(bad) == len(filler)
        with pytest.raises(ValueError) as e:
            gpu.parse_g(bad)
        assert f"byte {where + 1}:" in str(e.value) and repr(token[:64])[:-1] in str(e.value), (where, token, str(e.value))
        count, lines, offset = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        out = np.empty(len(filler))
        assert f(gpu.ctx, bad, len(bad), 0, out.ctypes.data_as(C.POINTER(C.c_double)), len(out), C.byref(count), C.byref(lines), C.byref(offset)) == BAD_ARG
        assert offset.value == where + 1
        assert token[:20].decode() in gpu.lib.gple_ctx_last_error(gpu.ctx).decode()
    # a 19-digit and a 64-byte token are fine
    values, _ = gpu.parse_g(with_token(with_token(filler, 77, b"1234567890123456789"), CHUNK - 30, b"0" * 63 + b"7"))
    assert 1234567890123456789.0 in values and 7.0 in values
    # of two malformed tokens the smaller offset, whichever chunk holds it
    two = with_token(with_token(filler, last_start + 20, b"abc"), CHUNK + 500, b"1e+")
    with pytest.raises(ValueError, match=f"byte {CHUNK + 501}:"):
        gpu.parse_g(two)
    # capacity one short: the count, nothing written; a null count
    count, offset = C.c_size_t(0), C.c_size_t(5)
    out = np.full(3000, -7.0)
    dp = out.ctypes.data_as(C.POINTER(C.c_double))
    assert f(gpu.ctx, filler, len(filler), 0, dp, 2999, C.byref(count), None, C.byref(offset)) == BAD_ARG
    assert count.value == 3000 and np.all(out == -7.0) and offset.value == C.c_size_t(-1).value
    assert f(gpu.ctx, filler, len(filler), 0, dp, 3000, None, None, None) == BAD_ARG
    assert f(gpu.ctx, None, 5, 0, dp, 3000, C.byref(count), None, None) == BAD_ARG and np.all(out == -7.0)
    assert f(gpu.ctx, filler, len(filler), 0, dp, 3000, C.byref(count), None, C.byref(offset)) == 0
    assert count.value == 3000 and np.all(out == 1.5) and offset.value == C.c_size_t(-1).value


# ---- the drivers ------------------------------------------------------------------------------------------------------------------------------
class WithoutParse:
    """the api with parse_g hidden: run_files then takes its host route"""

    def __init__(self, api):
        self._api = api

    def __getattr__(self, name):
        if name == "parse_g":
            raise AttributeError(name)
        return getattr(self._api, name)


def as_g(a):
    """float("%g" % v) of every entry (complex: of both parts)"""
    a = np.ascontiguousarray(a)
    flat = a.view(np.float64).ravel() if np.iscomplexobj(a) else a.ravel()
    return np.array([float("%g" % v) for v in flat]).view(a.dtype).reshape(a.shape)


def direct_records(gpu, model, num_pes, mass, x, p, states, seed, indices=None, **kw):
    """reconstruct() on each of `states` in turn with run_files' carry: the previous hyper-parameters, the first state's energy, seed + index"""
    import torch
    from gaussian_process_liouville_equation_amd import reconstruct as R
    state = R.State(gpu, num_pes, model, x, p, mass)
    recs, hyper, energy = [], None, None
    for index, rho in zip(indices or range(len(states)), states):
        rec = R.reconstruct(gpu, state, torch.from_numpy(np.ascontiguousarray(rho)).cuda(), seed=seed + index, start=hyper, initial_energy=energy, **kw)
        hyper, energy = rec["hyper"], rec["initial_energy"]
        recs.append(rec)
    return recs


def assert_same_records(got, want):
    """bit for bit (a NaN equals the same NaN: a search that fails on these coarse states may leave one)"""
    bits = lambda v: np.asarray(v, dtype=np.float64).view(np.uint64)
    assert len(got) == len(want)
    for a, b in zip(got, want):
        for key in KEYS + ("initial_energy",):
            assert np.array_equal(bits(a[key]), bits(b[key])), key
        assert all(np.array_equal(u, v) for u, v in zip(a["cells"], b["cells"]))


def test_run_files_on_an_mqcl_directory(gpu, tmp_path):
    from gaussian_process_liouville_equation_amd import exact_mqcl as EM, reconstruct as R
    kw = dict(dx=0.125, dt=1.0, xmin=-10.0, xmax=10.0, x0=-3.0, output_time=20.0)
    states = []
    res = EM.run(gpu, model=1, num_pes=2, ln_energy=0.0, out_dir=str(tmp_path / "run"), write_phase="text", max_outputs=3,
                 on_output=lambda t, adia: states.append(np.array(adia)), **kw)
    s = res["setup"]
    assert s["n_grids"] == 161 and len(states) == 4
    fit = dict(n_points=37, maxeval=60)
    recs = R.run_files(gpu, str(tmp_path / "run"), out_dir=str(tmp_path / "recon"), model=1, num_pes=2, mass=s["mass"], seed=11, **fit)
    assert [r["index"] for r in recs] == [0, 1, 2, 3] and [r["t"] for r in recs] == [float("%g" % r["t"]) for r in res["records"]]
    x, p = as_g(s["x"]), as_g(s["p"])
    rounded = [as_g(z) for z in states]
    want = direct_records(gpu, 1, 2, s["mass"], x, p, rounded, 11, **fit)
    assert_same_records(recs, want)
    # log.txt and choose.txt read back to the records
    log = np.loadtxt(tmp_path / "recon" / "log.txt", ndmin=2)
    assert log.shape[0] == 4
    for row, r in zip(log, recs):
        assert np.array_equal(row, [float(v) for v in R.log_line(r["t"], r).split()])
        assert row[0] == r["t"] and row[1] == float("%.16g" % r["nlml"]) and np.array_equal(row[2:18], [float("%.16g" % v) for v in r["hyper"].ravel()])
    blocks = (tmp_path / "recon" / "choose.txt").read_text().split("\n\n")[:-1]
    assert len(blocks) == 4
    for block, r in zip(blocks, recs):
        for line, feat in zip(block.split("\n"), r["features"]):
            assert np.array_equal(np.array(line.split(), dtype=float), as_g(feat).ravel())
    # the host route (float() per token, a numpy state): the same records
    assert_same_records(R.run_files(WithoutParse(gpu), str(tmp_path / "run"), model=1, num_pes=2, mass=s["mass"], seed=11, **fit), want)
    # one output alone (main_screenshot.cpp): the third record of a run that starts there — default start values, its own energy, seed + 2 —
    # and the first two blocks are not read at all; two outputs: the second starts from the first's hyper-parameters
    assert_same_records(R.run_files(gpu, str(tmp_path / "run"), model=1, num_pes=2, mass=s["mass"], seed=11, outputs=[2], **fit),
                        direct_records(gpu, 1, 2, s["mass"], x, p, rounded[2:3], 11, indices=[2], **fit))
    assert_same_records(R.run_files(gpu, str(tmp_path / "run"), model=1, num_pes=2, mass=s["mass"], seed=11, outputs=[3, 1], **fit),
                        direct_records(gpu, 1, 2, s["mass"], x, p, [rounded[1], rounded[3]], 11, indices=[1, 3], **fit))
    # a block of another grid is told by its counts
    (tmp_path / "run" / "x.txt").write_text("".join("%g\n" % v for v in s["x"][:-1]))
    with pytest.raises(ValueError, match="output 0"):
        R.run_files(gpu, str(tmp_path / "run"), model=1, num_pes=2, mass=s["mass"], **fit)


def test_run_files_on_a_dvr_directory(gpu, tmp_path):
    """three levels, n = 96 with 80 momenta.  exact.run does not hand its Wigner densities out, so the state of the direct call is the file read
    with Python's float() — float("%g" % v) of the run's state, given that the file holds "%g" % v (tests/test_gpu_format.py)"""
    from gaussian_process_liouville_equation_amd import exact, reconstruct as R
    s = exact.setup(-1.0, dx=0.25, xmin=-12.0, xmax=11.75)
    assert s["n_grids"] == 96
    p = np.linspace(s["p"][0], s["p"][-1], 80)
    res = exact.run(gpu, model=exact.DAC, num_pes=3, boundary=exact.PERIODIC, ln_energy=-1.0, dx=0.25, xmin=-12.0, xmax=11.75, max_outputs=3,
                    out_dir=str(tmp_path / "run"), write_phase="text", p_grid=p)
    assert len(res["records"]) == 3
    fit = dict(n_points=37, maxeval=60)
    recs = R.run_files(gpu, str(tmp_path / "run"), model=exact.DAC, num_pes=3, mass=s["mass"], seed=3, **fit)
    assert [r["index"] for r in recs] == [0, 1, 2] and recs[0]["hyper"].shape == (9, 4)
    blocks = [b for b in (tmp_path / "run" / "phase.txt").read_bytes().split(b"\n\n") if b.strip()]
    states = [np.array([float(t) for t in b.split()]).view(np.complex128).reshape(3, 3, 96, 80) for b in blocks]
    assert_same_records(recs, direct_records(gpu, exact.DAC, 3, s["mass"], as_g(s["x"]), as_g(p), states, 3, **fit))
    assert_same_records(R.run_files(WithoutParse(gpu), str(tmp_path / "run"), model=exact.DAC, num_pes=3, mass=s["mass"], seed=3, **fit), recs)
