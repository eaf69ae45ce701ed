"""GPU: gple_mqcl_evolve at every workgroup size of its X and P pass, n = 4 .. 4096, and gple_mqcl_observe / gple_mqcl_transform beyond one trip
of their loops (csrc/gple_mqcl.hip), against the numpy restatement tests/mqcl_numpy.py.

Up to n = 2049 the whole coupled step is restated.  Beyond that the restatement is too slow and too large, so the two decoupled limits are
restated instead: with mass = MN.DECOUPLE the R propagator is the identity and every x row evolves alone under Q and P; with length_p =
MN.DECOUPLE every p column evolves alone under Q and R.  The device still runs all of its passes (the idle one with psi = 1); 32 sampled rows or
columns are restated exactly, and the sum of the trace along every row or column, conserved by the equation, covers every workgroup.
tests/test_mqcl_host.py pins both claims on the restatement itself.

Which case reaches which instantiation mqcl_{x,p}pass_kernel<num_pes, NT> (both kernels run in every evolve call):
    <2, 64>    test_coupled, two levels, n = 4 .. 256           <3, 64>    test_coupled, three levels, n = 4 .. 256
    <2, 256>   test_coupled, two levels, n = 257, 1024          <3, 256>   test_coupled, three levels, n = 257
    <2, 512>   test_coupled (2, 1025); test_decoupled (2, 2048) <3, 512>   test_coupled (3, 1025)
    <2, 1024>  test_coupled (2, 2049); test_decoupled (2, 2049), (2, 4096); test_zero_time_step_at_the_largest_grid
    <3, 1024>  test_decoupled (3, 2049), (3, 4096)
The fourth register slot of a thread (indices 3 NT .. 4 NT - 1) is occupied at n = 256, 1024, 2048 and 4096 only."""
import numpy as np
import pytest

from tests import mqcl_numpy as MN
from tests.test_gpu_mqcl import EVOLVE_TOL, gaussian, grid, rel

pytestmark = pytest.mark.gpu

# (num_pes, model, n, steps): the edges of the FFT length (2n - 1 = 255 at n = 128, M = 512 at 129), of the slot occupancy (n = M / 2 with four
# full slots at 256 and 1024), of the 32-tiles of the transpose, the API minimum n = 4 (M = 8: one butterfly stage between the fused ones), and
# the smallest grid of each larger workgroup (257, 1025, 2049)
COUPLED = ([(2, 1, n, 3) for n in (4, 5, 7, 8, 9, 16, 17, 31, 32, 33, 128, 129, 256, 257)] + [(3, 3, n, 3) for n in (4, 5, 33, 129, 256, 257)] +
           [(2, 1, 1024, 2), (2, 1, 1025, 2), (3, 3, 1025, 2), (2, 1, 2049, 1)])


@pytest.mark.parametrize("num_pes, model, n, steps", COUPLED)
def test_coupled(gpu, num_pes, model, n, steps):
    """the full restatement; two steps run the inner [R Q Q R] pass and both end passes.  (2, 2049) is the one coupled comparison on the
    NT = 1024 kernels, the only ones that spill registers: its restatement is most of this file's wall time"""
    x, p, lx, lp = grid(n)
    rho = MN.random_hermitian(num_pes, n, np.random.default_rng(1000 * num_pes + n))
    dev = gpu.mqcl_evolve(num_pes, model, x, p, rho, 2000.0, lx, lp, 0.25, steps)
    ref = MN.evolve(rho, MN.Bases(x, model, num_pes), p, 2000.0, lx, lp, 0.25, steps)
    d = rel(dev, ref)
    print(f"coupled num_pes {num_pes} n {n} steps {steps}: err {d:.3e} err/tol {d / EVOLVE_TOL:.3f}")
    assert d <= EVOLVE_TOL, d
    assert np.array_equal(dev, np.conj(np.swapaxes(dev, 0, 1)))
    for a in range(num_pes):
        assert (dev[a, a].imag == 0.0).all()


def device_state(num_pes, n, seed):
    """a random Hermitian state with real diagonal planes, built on the device: the host never holds it"""
    import torch

    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    z = torch.view_as_complex(torch.randn((num_pes, num_pes, n, n, 2), dtype=torch.float64, device="cuda", generator=g))
    rho = torch.empty_like(z)
    for a in range(num_pes):
        rho[a, a] = z[a, a].real
        for b in range(a + 1, num_pes):
            rho[a, b] = 0.5 * (z[a, b] + torch.conj_physical(z[b, a]))
            rho[b, a] = torch.conj_physical(rho[a, b])
    return rho


def sampled(n, seed, count=32):
    """the borders of the transpose's 32-tiles, its ragged last tile, and seeded draws from the rest"""
    fixed = np.array([0, 1, 31, 32, 33, n - 33, n - 32, n - 2, n - 1])
    rest = np.random.default_rng(seed).permutation(np.setdiff1d(np.arange(n), fixed))[:count - len(fixed)]
    return np.sort(np.concatenate([fixed, rest]))


def trace_sums(rho, dim):
    """per row (dim = 1: over p) or per column (dim = 0: over x): sum_a Re rho_aa, each plane summed on the device in float64"""
    return sum(rho[a, a].real.sum(dim=dim).cpu().numpy() for a in range(rho.shape[0]))


def exactly_hermitian(rho):
    import torch

    num_pes = rho.shape[0]
    return (all(bool((rho[a, a].imag == 0.0).all()) for a in range(num_pes)) and
            all(torch.equal(rho[b, a], torch.conj_physical(rho[a, b])) for a in range(num_pes) for b in range(a + 1, num_pes)))


@pytest.mark.parametrize("axis", ["rows", "columns"])
@pytest.mark.parametrize("num_pes, n", [(2, 2048), (2, 2049), (3, 2049), (2, 4096), (3, 4096)])
def test_decoupled(gpu, num_pes, n, axis):
    """rows: mass = DECOUPLE, the P pass does the work; columns: length_p = DECOUPLE, the X pass does.  The conservation bound 1e-11 of the largest
    sum stands against the restatement's own drift on the sampled lines, printed beside the device's over all lines (measured at n = 4096:
    3.3e-15 and 6.2e-15)"""
    import torch

    model = 1 if num_pes == 2 else 3
    steps, dt, mass = 2, 2.0, 2000.0
    x, p, lx, lp = grid(n)
    rho = device_state(num_pes, n, 7 * n + num_pes)
    idx = sampled(n, n + num_pes)
    pick = torch.from_numpy(idx).cuda()
    take = (lambda r: r[:, :, pick, :]) if axis == "rows" else (lambda r: r[:, :, :, pick])
    dim = 1 if axis == "rows" else 0
    start = take(rho).cpu().numpy()
    sums0 = trace_sums(rho, dim)
    dx_, dp_ = torch.from_numpy(x).cuda(), torch.from_numpy(p).cuda()
    torch.cuda.synchronize()  # the library runs on its own stream
    if axis == "rows":
        gpu.mqcl_evolve(num_pes, model, dx_, dp_, rho, MN.DECOUPLE, lx, lp, dt, steps)
        restate = lambda freq: MN.evolve_rows(start, x[idx], p, model, num_pes, lx, lp, dt, steps, freq=freq)
    else:
        gpu.mqcl_evolve(num_pes, model, dx_, dp_, rho, mass, lx, MN.DECOUPLE, dt, steps)
        bases = MN.Bases(x, model, num_pes)
        restate = lambda freq: MN.evolve_columns(start, bases, p[idx], mass, lx, dt, steps, freq=freq)
    torch.cuda.synchronize()
    dev = take(rho).cpu().numpy()
    sums1 = trace_sums(rho, dim)
    ref = restate(MN.ref_freq)
    d = rel(dev, ref)
    moved = rel(start, ref)
    host_sums = lambda r: sum(r[a, a].real.sum(axis=dim) for a in range(num_pes))
    drift = np.abs(sums1 - sums0).max() / np.abs(sums0).max()
    ref_drift = np.abs(host_sums(ref) - host_sums(start)).max() / np.abs(sums0).max()
    print(f"decoupled {axis} num_pes {num_pes} n {n}: err {d:.3e} err/tol {d / EVOLVE_TOL:.3f} moved {moved:.2e} drift {drift:.2e} "
          f"(restatement, sampled: {ref_drift:.2e})")
    assert d <= EVOLVE_TOL, d
    assert moved > 1e-2  # the surviving propagator is not the identity
    if n % 2:
        other = rel(dev, restate(MN.fftfreq))
        print(f"    fftfreq restatement: {other:.3e}")
        assert other > 1000 * EVOLVE_TOL, other
    assert drift <= 1e-11, drift
    assert exactly_hermitian(rho)


def test_zero_time_step_at_the_largest_grid(gpu):
    """dt = 0: every phase is zero and every pass of a coupled step must hand the whole 4096 x 4096 state back (three shifts of four
    length-8192 FFTs per plane, the rotations, the transposes)"""
    import torch

    num_pes, model, n = 2, 1, 4096
    x, p, lx, lp = grid(n)
    rho = device_state(num_pes, n, 5)
    start = rho.clone()
    dx_, dp_ = torch.from_numpy(x).cuda(), torch.from_numpy(p).cuda()
    torch.cuda.synchronize()
    gpu.mqcl_evolve(num_pes, model, dx_, dp_, rho, 2000.0, lx, lp, 0.0, 1)
    torch.cuda.synchronize()
    d = float((rho - start).abs().max() / start.abs().max())
    print(f"dt = 0 num_pes {num_pes} n {n}: err {d:.3e} err/tol {d / EVOLVE_TOL:.3f}")
    assert d <= EVOLVE_TOL, d
    assert exactly_hermitian(rho)


@pytest.mark.parametrize("n", [257, 600])
@pytest.mark.parametrize("num_pes, model", [(2, 1), (3, 3)])
def test_observe_beyond_one_trip(gpu, num_pes, model, n):
    """n > 256: the j += 256 loop of the row kernel and the i += 256 loop of the final sum take a second (n = 600: a third, ragged) trip"""
    x, p, _, _ = grid(n)
    dx, dp = x[1] - x[0], p[1] - p[0]
    bases = MN.Bases(x, model, num_pes)
    rho = MN.transform(gaussian(num_pes, x, p) * (1.0 + 0.0j), bases, MN.ADIABATIC, MN.DIABATIC)
    adia, av, pops = gpu.mqcl_observe(num_pes, model, x, p, rho, 2000.0, dx, dp)
    radia, rav, rpops = MN.observe(rho, bases, x, p, 2000.0, dx, dp)
    print(f"observe num_pes {num_pes} n {n}: adia {rel(adia, radia):.2e} averages {np.abs(av - rav).max() / np.abs(rav).max():.2e} "
          f"populations {np.abs(pops - rpops).max() / np.abs(rpops).max():.2e}")
    assert rel(adia, radia) <= 1e-13
    assert np.abs(av - rav).max() <= 1e-12 * np.abs(rav).max(), (av, rav)
    assert np.abs(pops - rpops).max() <= 1e-13 * np.abs(rpops).max()
    adia2, av2, pops2 = gpu.mqcl_observe(num_pes, model, x, p, rho, 2000.0, dx, dp)
    assert np.array_equal(adia, adia2) and np.array_equal(av, av2) and np.array_equal(pops, pops2)


@pytest.mark.parametrize("num_pes, model", [(2, 1), (3, 3)])
def test_transforms_beyond_one_row_per_block(gpu, num_pes, model):
    """n = 300: a 256-thread block of the transform kernel straddles two x rows, and the last block is ragged"""
    n = 300
    x, _, _, _ = grid(n)
    rho = MN.random_hermitian(num_pes, n, np.random.default_rng(300 + num_pes))
    bases = MN.Bases(x, model, num_pes)
    for frm in range(3):
        src = gpu.mqcl_transform(num_pes, model, x, rho, MN.DIABATIC, frm)
        for to in range(3):
            dev = gpu.mqcl_transform(num_pes, model, x, src, frm, to)
            ref = MN.transform(rho, bases, MN.DIABATIC, to)
            # a basis vector is defined up to its sign: align the restatement's off-diagonal rows (a, b, x_i), as test_gpu_mqcl.test_transforms
            for a in range(num_pes):
                for b in range(num_pes):
                    if a != b:
                        sgn = np.where(np.einsum("ij,ij->i", dev[a, b], np.conj(ref[a, b])).real < 0, -1.0, 1.0)
                        ref[a, b] *= sgn[:, None]
            print(f"transform num_pes {num_pes} n {n} {frm} -> {to}: {rel(dev, ref):.2e}")
            assert rel(dev, ref) <= 1e-13, (frm, to, rel(dev, ref))
            assert np.array_equal(dev, np.conj(np.swapaxes(dev, 0, 1)))
