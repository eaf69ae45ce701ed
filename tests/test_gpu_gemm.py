"""GPU: the fp64 MFMA GEMM family of the fit (csrc/gple_gemm.hip) on its own, through the library's diagnostic entry
gple_debug_gemm (not part of include/gple.h): every tile kernel (32 = split-k, 64 = 4-slab ring, 128 = double-buffered), every
operand layout it is instantiated for, the triangular k-ranges of the merge tree / T^T T, lower-only results and beta != 0,
against numpy in double precision.  The fits exercise these kernels only at the shapes a fit produces."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K_FULL, K_GE_N, K_LE_M, K_GE_MAX_MN = 0, 1, 2, 3


def _gemm(gpu, A, B, C, ak, bk, ct, alpha, beta, krange, lower_only, tile):
    """A: (M, K) logical, B: (N, K) logical, C: (M, N) logical; stored per the layout flags"""
    lib = gpu.lib
    if not hasattr(lib, "gple_debug_gemm"):
        pytest.fail("libgple_hip.so lacks gple_debug_gemm")
    lib.gple_debug_gemm.restype = ctypes.c_int
    M, K = A.shape
    N = B.shape[0]
    As = np.ascontiguousarray(A) if ak else np.asfortranarray(A)  # kmajor: element (r, k) at k + r * ld
    Bs = np.ascontiguousarray(B) if bk else np.asfortranarray(B)
    Cs = np.ascontiguousarray(C) if ct else np.asfortranarray(C)  # c_trans: C(m, n) at n + m * ldc
    Cs = Cs.copy(order="C" if ct else "F")
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = lib.gple_debug_gemm(gpu.ctx, p(As), ctypes.c_long(K if ak else M), int(ak), p(Bs), ctypes.c_long(K if bk else N), int(bk), p(Cs),
                             ctypes.c_long(N if ct else M), int(ct), M, N, K, ctypes.c_double(alpha), ctypes.c_double(beta), krange, int(lower_only), tile)
    assert rc == 0, rc
    return np.array(Cs)


def _reference(A, B, C, alpha, beta, krange, lower_only, tile):
    M, K = A.shape
    N = B.shape[0]
    Am, Bm = A.copy(), B.copy()
    k = np.arange(K)
    if krange == K_GE_N:  # B(n, k) != 0 only for k >= n
        Bm = Bm * (k[None, :] >= np.arange(N)[:, None])
    elif krange == K_LE_M:  # A(m, k) != 0 only for k <= m
        Am = Am * (k[None, :] <= np.arange(M)[:, None])
    elif krange == K_GE_MAX_MN:
        Am = Am * (k[None, :] >= np.arange(M)[:, None])
        Bm = Bm * (k[None, :] >= np.arange(N)[:, None])
    out = alpha * (Am @ Bm.T) + beta * C
    if lower_only:  # tiles strictly above the block diagonal are not computed: compare the lower tiles only
        bt = 32 if tile == 32 else (128 if tile == 128 else 64)
        mi, ni = np.arange(M)[:, None] // bt, np.arange(N)[None, :] // bt
        return out, ni <= mi
    return out, np.ones((M, N), bool)


CASES = [
    # tile, ak, bk, ct, M, N, K, krange, lower_only, beta
    (32, False, False, False, 192, 128, 64, K_FULL, False, 0.0),     # K = 64 trailing update shape
    (32, False, False, False, 256, 256, 64, K_FULL, True, 1.0),      # ... as the factorisation calls it
    (32, False, True, False, 128, 128, 128, K_GE_N, False, 0.0),     # W = L21 T11
    (32, False, True, False, 256, 256, 256, K_LE_M, False, 0.0),     # T21 = -T22 W
    (32, False, True, False, 96, 160, 48, K_FULL, False, 0.5),       # ragged in 32s, fewer k-groups than waves
    (64, False, False, False, 256, 192, 256, K_FULL, True, 1.0),     # outer update
    (64, False, True, False, 256, 256, 256, K_LE_M, False, 0.0),
    (64, False, True, False, 256, 256, 256, K_GE_N, False, 0.0),
    (64, True, True, False, 256, 256, 256, K_GE_MAX_MN, True, 0.0),  # T^T T
    (64, False, False, True, 128, 192, 80, K_FULL, False, 0.0),
    (64, False, True, True, 128, 128, 128, K_LE_M, False, 0.0),      # few-rows predict
    (128, False, False, False, 256, 384, 144, K_FULL, False, 0.0),   # derivative products
    (128, True, True, False, 256, 256, 256, K_GE_MAX_MN, True, 0.0),
    (128, False, True, False, 256, 256, 256, K_LE_M, False, 2.0),
    # more shapes of the 128-tile kernel (round 4: one and two slabs, k-ranges with row-contiguous operands, lower tiles, the XCD-aware tile order)
    (128, False, False, True, 256, 128, 208, K_FULL, False, 0.0),
    (128, False, False, False, 128, 256, 16, K_FULL, False, 1.5),    # one slab
    (128, False, False, False, 384, 128, 32, K_FULL, False, 0.0),    # two slabs
    (128, False, False, False, 384, 384, 384, K_LE_M, False, 0.0),   # k-range by row block
    (128, False, False, False, 384, 384, 384, K_GE_N, False, 0.0),   # k-range from the column block on
    (128, False, False, False, 512, 512, 96, K_FULL, True, 1.0),     # lower tiles only
    (128, False, False, False, 1024, 1024, 512, K_FULL, False, 0.0), # the XCD-aware tile order (8 | N-tiles)
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "t%d_%s%s%s_%dx%dx%d_kr%d_lo%d" % (c[0], "k" if c[1] else "r", "k" if c[2] else "r", "t" if c[3] else "n", c[4], c[5], c[6], c[7], c[8]))
def test_gemm_tile_kernels(gpu, case):
    tile, ak, bk, ct, M, N, K, krange, lower_only, beta = case
    rng = np.random.default_rng(M + 7 * N + 13 * K + tile)
    A, B, C = rng.standard_normal((M, K)), rng.standard_normal((N, K)), rng.standard_normal((M, N))
    if krange in (K_GE_N, K_GE_MAX_MN):
        B = B * (np.arange(K)[None, :] >= np.arange(N)[:, None])  # the operand really is triangular (the kernel may skip or not)
    if krange in (K_LE_M,):
        A = A * (np.arange(K)[None, :] <= np.arange(M)[:, None])
    if krange == K_GE_MAX_MN:
        A = A * (np.arange(K)[None, :] >= np.arange(M)[:, None])
    alpha = -1.0 if lower_only else 0.75
    got = _gemm(gpu, A, B, C, ak, bk, ct, alpha, beta, krange, lower_only, tile)
    ref, mask = _reference(A, B, C, alpha, beta, krange, lower_only, tile)
    scale = np.abs(A) @ np.abs(B).T * abs(alpha) + abs(beta) * np.abs(C)
    err = np.abs(got - ref)[mask] / np.maximum(scale[mask], 1e-300)
    assert err.max() <= 4 * 2.3e-16 * np.sqrt(K), err.max()
    if lower_only:  # tiles that are not computed keep their input
        assert np.array_equal(got[~mask], C[~mask])


# ---- the family as the fits call it: windows of larger buffers, batches, operands and results that border on memory nobody may touch ----------
# gple_debug_gemm above passes tight operands at their buffers' origins, one item, a finite C.  The fits (csrc/gple_capi.hip, gple_chol.hip) never do:
# every operand is a sub-block of an n_total-leading-dimension matrix, the derivative products run as batches of 2 / 3 with strideB = 0, and
# beta == 0 is relied upon not to read C (the session runs with GPLE_POISON_T=1: an unwritten block is NaN).  gple_debug_gemm_strided takes the whole
# buffers, so a test sees every element a launch may not read (NaN there must not reach the result) or write (a sentinel there must keep its bits).
def _w(row, col, ld, stride=0, item=0):
    """(element offset, leading dimension, batch stride) of a window at (row, col) of the item-th ld x ld matrix; row/col: contiguous / strided index"""
    return (item * ld * ld + row + col * ld, ld, stride)


STRIDED = {
    # complex derivative products E = A M_a, F = B M_b in their smallest form (complex_fit_derivatives: Np = 256, n_total = 512, three parameters a launch):
    # A a quadrant of each item's 512 x 512 dC, B a column half of the one M (strideB = 0), C the E / F half of each item's [E | F]
    "complex_deriv": dict(counts=(3 * 512 * 512, 512 * 512, 3 * 2 * 256 * 512), calls=[
        dict(A=_w(256, 256, 512, 512 * 512), B=_w(0, 256, 512), C=(0, 256, 2 * 256 * 512), M=256, N=512, K=256, batch=3),
        dict(A=_w(0, 256, 512, 512 * 512), B=_w(0, 0, 512), C=(256 * 512, 256, 2 * 256 * 512), M=256, N=512, K=256, batch=3)]),
    # real derivative products dK_d W (real_fit_derivatives: two length parameters a launch, or one of them twice over when the other is masked out)
    "real_deriv_strideA": dict(counts=(2 * 384 * 384, 384 * 384, 2 * 384 * 384), calls=[
        dict(A=_w(64, 64, 384, 384 * 384), B=_w(0, 128, 384), C=_w(128, 64, 384, 384 * 384), M=256, N=256, K=256, batch=2)]),
    "real_deriv_strideA0": dict(counts=(384 * 384, 384 * 384, 2 * 384 * 384), calls=[
        dict(A=_w(64, 64, 384, 0), B=_w(0, 128, 384), C=_w(128, 64, 384, 384 * 384), M=256, N=256, K=256, batch=2)]),
    # sub-blocks of the factorisation and the block-row inverse: origin (192, 192) — an odd multiple of 64, as at a fork point — of a 640-column matrix
    "chol_K_LE_M": dict(counts=(640 * 640,) * 3, tiles=(32, 64), calls=[
        dict(A=_w(192, 192, 640), B=_w(192, 192, 640), C=_w(192, 192, 640), M=256, N=256, K=256, bk=True, krange=K_LE_M)]),
    "chol_K_GE_N": dict(counts=(640 * 640,) * 3, tiles=(32, 64), calls=[
        dict(A=_w(192, 192, 640), B=_w(192, 192, 640), C=_w(192, 192, 640), M=256, N=256, K=256, bk=True, krange=K_GE_N)]),
    "chol_K_GE_MAX_MN": dict(counts=(640 * 640,) * 3, tiles=(32, 64), calls=[  # T^T T (k-major A: the split-k request runs on 64-tiles)
        dict(A=_w(192, 192, 640), B=_w(192, 192, 640), C=_w(192, 192, 640), M=256, N=256, K=256, ak=True, bk=True, krange=K_GE_MAX_MN, lower_only=True)]),
    "chol_lower_beta1": dict(counts=(640 * 640,) * 3, tiles=(32, 64), calls=[  # trailing update
        dict(A=_w(192, 192, 640), B=_w(192, 192, 640), C=_w(192, 192, 640), M=256, N=256, K=64, alpha=-1.0, beta=1.0, lower_only=True)]),
}
_STRIDED_DATA = {}


def _index(window, batch, rows, cols, rows_contiguous):
    """flat element index of the logical element (item, r, c) of a window"""
    off, ld, stride = window
    z, r, c = np.arange(batch)[:, None, None] * stride, np.arange(rows)[None, :, None], np.arange(cols)[None, None, :]
    return off + z + (r + c * ld if rows_contiguous else c + r * ld)


def _strided_data(name):
    """per call of a case, made once and shared by the tile sizes: operand buffers that are NaN outside the windows the product is defined on, the C
    window's finite input, the longdouble product and its scale"""
    if name in _STRIDED_DATA:
        return _STRIDED_DATA[name]
    spec = STRIDED[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    base = [rng.standard_normal(n) for n in spec["counts"][:2]]
    out = []
    for call in spec["calls"]:
        M, N, K, batch = call["M"], call["N"], call["K"], call.get("batch", 1)
        ak, bk, ct, krange = call.get("ak", False), call.get("bk", False), call.get("ct", False), call.get("krange", K_FULL)
        alpha, beta = call.get("alpha", 0.75), call.get("beta", 0.0)
        ia, ib, ic = _index(call["A"], batch, M, K, not ak), _index(call["B"], batch, N, K, not bk), _index(call["C"], batch, M, N, not ct)
        assert ia.max() < spec["counts"][0] and ib.max() < spec["counts"][1] and ic.max() < spec["counts"][2]
        A, B = base[0][ia], base[1][ib]
        k = np.arange(K)
        if krange in (K_GE_N, K_GE_MAX_MN):  # the part a k-range excludes holds finite zeros (_reference: the kernel may skip them or not)
            B = B * (k[None, :] >= np.arange(N)[:, None])
        if krange == K_LE_M:
            A = A * (k[None, :] <= np.arange(M)[:, None])
        if krange == K_GE_MAX_MN:
            A = A * (k[None, :] >= np.arange(M)[:, None])
        Abuf, Bbuf = np.full(spec["counts"][0], np.nan), np.full(spec["counts"][1], np.nan)
        Abuf[ia], Bbuf[ib] = A, B
        Cwin = rng.standard_normal((batch, M, N))
        ref = alpha * np.matmul(A.astype(np.longdouble), B.astype(np.longdouble).transpose(0, 2, 1)) + beta * Cwin
        scale = abs(alpha) * np.matmul(np.abs(A), np.abs(B).transpose(0, 2, 1)) + abs(beta) * np.abs(Cwin)
        out.append(dict(call, batch=batch, ak=ak, bk=bk, ct=ct, krange=krange, alpha=alpha, beta=beta, lower_only=call.get("lower_only", False),
                        Abuf=Abuf, Bbuf=Bbuf, ic=ic, Cwin=Cwin, ref=ref, scale=scale))
    _STRIDED_DATA[name] = out
    return out


def _gemm_strided(gpu, d, Cbuf, tile):
    lib = gpu.lib
    if not hasattr(lib, "gple_debug_gemm_strided"):
        pytest.fail("libgple_hip.so lacks gple_debug_gemm_strided")
    fn = lib.gple_debug_gemm_strided
    operand = [ctypes.c_void_p, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_int]
    fn.argtypes = [ctypes.c_void_p] + 3 * operand + 4 * [ctypes.c_int] + 2 * [ctypes.c_double] + 3 * [ctypes.c_int]
    fn.restype = ctypes.c_int
    out = Cbuf.copy()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = fn(gpu.ctx, p(d["Abuf"]), d["Abuf"].size, *d["A"], int(d["ak"]), p(d["Bbuf"]), d["Bbuf"].size, *d["B"], int(d["bk"]), p(out), out.size, *d["C"], int(d["ct"]),
            d["batch"], d["M"], d["N"], d["K"], d["alpha"], d["beta"], d["krange"], int(d["lower_only"]), tile)
    assert rc == 0, rc
    return out


@pytest.mark.parametrize("name,tile", [(n, t) for n in STRIDED for t in STRIDED[n].get("tiles", (32, 64, 128))], ids=lambda v: str(v))
def test_gemm_on_windows_of_larger_buffers(gpu, name, tile):
    """every launch of a case: the windows hold the longdouble product (tolerance of test_gemm_tile_kernels), every other element of the C buffer —
    leading-dimension gap rows, the space between batch items, the other half of [E | F], tiles that lower_only skips — keeps its bits, NaN
    around the operand windows stays out of the result, and beta == 0 gives the same finite bits over a NaN C as over a finite one"""
    Cbuf = 1.0e6 + np.arange(STRIDED[name]["counts"][2], dtype=np.float64)  # the sentinel: finite, and a shifted copy would show
    bits = lambda a: a.view(np.uint64)
    for d in _strided_data(name):
        eff = 64 if tile == 32 and (d["ak"] or d["ct"]) else tile  # launch_gemm: layouts the split-k kernel is not instantiated for
        mi, ni = np.arange(d["M"])[:, None] // eff, np.arange(d["N"])[None, :] // eff
        computed = np.broadcast_to(ni <= mi if d["lower_only"] else np.ones((d["M"], d["N"]), bool), d["Cwin"].shape)
        written = np.zeros(Cbuf.size, bool)
        written[d["ic"][computed]] = True
        Cin = Cbuf.copy()
        Cin[d["ic"]] = d["Cwin"]
        got = _gemm_strided(gpu, d, Cin, tile)
        err = np.abs(got[d["ic"]] - d["ref"])[computed].astype(np.float64) / np.maximum(d["scale"][computed], 1e-300)
        print("%s tile %d: worst error / tolerance %.3f" % (name, tile, np.nanmax(err) / (4 * 2.3e-16 * np.sqrt(d["K"]))))
        assert np.all(np.isfinite(got[d["ic"]][computed]))
        assert err.max() <= 4 * 2.3e-16 * np.sqrt(d["K"]), err.max()
        assert np.array_equal(bits(got)[~written], bits(Cin)[~written]), int((bits(got) != bits(Cin))[~written].sum())
        if d["beta"] == 0.0:
            Cnan = Cbuf.copy()
            Cnan[d["ic"]] = np.nan
            got2 = _gemm_strided(gpu, d, Cnan, tile)
            assert np.all(np.isfinite(got2[written])) and np.array_equal(got2[written], got[written])
            assert np.array_equal(bits(got2)[~written], bits(Cnan)[~written])
        Cbuf = got  # the next launch of the case finds this one's result in the buffer and must leave it alone


def test_gemm_strided_refuses_windows_that_leave_their_buffers(gpu):
    """the diagnostic entry checks every window on the host: nothing that could read or write out of bounds is launched"""
    d = _strided_data("real_deriv_strideA")[0]
    Cbuf = np.zeros(STRIDED["real_deriv_strideA"]["counts"][2])
    _gemm_strided(gpu, d, Cbuf, 64)  # (the valid call; it also declares the argument types)
    fn = gpu.lib.gple_debug_gemm_strided
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    # a column too far for the last item; a batch stride on a one-item buffer; items of C that overlap; an origin no 32-byte load can start at
    for key, bad in (("A", (64 + 129 * 384, 384, 384 * 384)), ("B", (0, 384, 384 * 384)), ("C", (128 + 64 * 384, 384, 256 * 384 - 4)), ("A", (66, 384, 0))):
        bd = dict(d, **{key: bad})
        out = Cbuf.copy()
        rc = fn(gpu.ctx, p(bd["Abuf"]), bd["Abuf"].size, *bd["A"], 0, p(bd["Bbuf"]), bd["Bbuf"].size, *bd["B"], 0, p(out), out.size, *bd["C"], 0,
                2, 256, 256, 256, 1.0, 0.0, K_FULL, 0, 64)
        assert rc != 0 and np.array_equal(out, Cbuf), (key, rc)


def test_gemm_split_k_is_deterministic(gpu):
    """the four waves' partial sums meet in LDS in a fixed order: two runs agree bit for bit"""
    rng = np.random.default_rng(3)
    A, B, C = rng.standard_normal((128, 512)), rng.standard_normal((128, 512)), np.zeros((128, 128))
    r1 = _gemm(gpu, A, B, C, False, True, False, 1.0, 0.0, K_FULL, False, 32)
    r2 = _gemm(gpu, A, B, C, False, True, False, 1.0, 0.0, K_FULL, False, 32)
    assert np.array_equal(r1, r2)

