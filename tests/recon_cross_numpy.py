"""Independent numpy restatement of the grid reconstruction with the cross-term ARD kernel (the default build of test/gpr.cpp:99-103,
313-321, 436-452; gple_grid_reconstruct_cross) for the tests — a helper, not collected by pytest.  Written from the formulas:
the kernel k = w_g^2 exp(-Q / 2), Q = (a dx + c dp)^2 + (b dp)^2 of the weight matrix W = [[a, 0], [c, b]], hyper = (w_d, w_g, a, c, b); the
direct sum over the training points in longdouble, entry by entry on the tensor grid; the tile-centred split the device kernel uses, with
its range rule; and the entry bound 4 eps [(N + 8) S + S_A] + eps max|mu| with S_A weighted by the exponents of whichever form a tile takes.
The six sums are tests/recon_numpy.sums_of on the result."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

LD = np.longdouble
EPS = 2.0 ** -53
TILE = 64     # the device kernel's tile edge and
LIMIT = 6.0   # its L: |a| max|u| and |c| max|v| of a tile at most L, or the tile takes the plain path


def gram(hyper, A, B, dtype=LD):
    """w_g^2 exp(-((a dx + c dp)^2 + (b dp)^2) / 2) between the points A (n, 2) and B (m, 2): the ARD kernel alone"""
    _, wg, a, c, b = [dtype(h) for h in hyper]
    A, B = A.astype(dtype), B.astype(dtype)
    dx, dp = A[:, None, 0] - B[None, :, 0], A[:, None, 1] - B[None, :, 1]
    lin, bd = a * dx + c * dp, b * dp
    return wg * wg * np.exp(-(lin * lin + bd * bd) / 2)


def train_gram(hyper, X, dtype=LD):
    return gram(hyper, X, X, dtype) + dtype(hyper[0]) ** 2 * np.eye(len(X), dtype=dtype)


def tiles_of(n, tile=TILE):
    """[(first row, one past the last row, centre row)] of the tiles along one axis: the centre is a grid point, clamped to the grid"""
    return [(r0, min(r0 + tile, n), min(r0 + tile // 2, n - 1)) for r0 in range(0, n, tile)]


def tile_ranges(hyper, x, p, tile=TILE):
    """A_U (tiles along x,) = |a| max|u| and C_V (tiles along p,) = |c| max|v| in the device's own float64 arithmetic"""
    a, c = float(hyper[2]), float(hyper[3])
    AU = np.array([abs(a) * np.abs(x[r0:r1] - x[rc]).max() for r0, r1, rc in tiles_of(len(x), tile)])
    CV = np.array([abs(c) * np.abs(p[r0:r1] - p[rc]).max() for r0, r1, rc in tiles_of(len(p), tile)])
    return AU, CV


def centred_tiles(hyper, x, p, tile=TILE, limit=LIMIT):
    """(tiles along x, tiles along p) bool: the tile takes the centred form (both ranges inside the limit)"""
    AU, CV = tile_ranges(hyper, x, p, tile)
    return (AU[:, None] <= limit) & (CV[None, :] <= limit)


def split_exponents(hyper, X, u, v, xc, pc, dtype=np.float64):
    """the three exponents of the centred form for the rows u = x_a - x_c, the columns v = p_b - p_c and the points X around the centre
    (x_c, p_c): x operand (rows, N), p operand (columns, N), cell (rows, columns); their sum over a (row, column, point) is -Q / 2"""
    _, _, a, c, b = [dtype(h) for h in hyper]
    X, u, v = X.astype(dtype), u.astype(dtype), v.astype(dtype)
    t = dtype(pc) - X[:, 1]
    g = a * (dtype(xc) - X[:, 0]) + c * t
    q = g * g / 4
    ex = -(a * u[:, None] + g[None, :]) ** 2 / 2 + q[None, :]
    ep = (-(c * v[:, None] + g[None, :]) ** 2 / 2 + q[None, :]) - (b * (v[:, None] + t[None, :])) ** 2 / 2
    cell = -(a * c * u[:, None] * v[None, :])
    return ex, ep, cell


def _block(hyper, X, w, x, p, rows, cols, xc, pc, centred):
    """one block of cells: (mu longdouble, S, S_A) with the weights of the form its tile takes"""
    _, _, a, c, b = [LD(h) for h in hyper]
    dx, dp = x[rows].astype(LD)[:, None, None] - X[None, None, :, 0].astype(LD), p[cols].astype(LD)[None, :, None] - X[None, None, :, 1].astype(LD)
    lin, bd = a * dx + c * dp, b * dp
    half_q = (lin * lin + bd * bd) / 2
    k = np.exp(-half_q)
    mu = (k * w.astype(LD)).sum(axis=-1)
    kabs = k.astype(np.float64) * np.abs(w)
    if centred:
        ex, ep, cell = split_exponents(hyper, X, x[rows] - xc, p[cols] - pc, xc, pc)
        weight = np.abs(ex)[:, None, :] + np.abs(ep)[None, :, :] + np.abs(cell)[:, :, None]
    else:
        weight = half_q.astype(np.float64)
    return mu, kabs.sum(axis=-1), (kabs * weight).sum(axis=-1)


def predict_plane(hyper, X, b, x, p, c=1.0, tile=TILE, limit=LIMIT, threads=16, block=1 << 20):
    """c k((x_a, p_b), X) b on the tensor grid as the direct sum in longdouble, the entry bound 4 eps [(N + 8) S + S_A] + eps max|mu|
    (S = sum |c w_g^2 b_i| k_i; S_A the same weighted by |x exponent| + |p exponent| + |a c u v| in a centred tile and by Q / 2 in a plain
    one), and which tiles are centred"""
    X = np.ascontiguousarray(X, dtype=np.float64)
    w = float(c) * float(hyper[1]) ** 2 * np.asarray(b, dtype=np.float64)
    centred = centred_tiles(hyper, x, p, tile, limit)
    nx, np_ = len(x), len(p)
    mu, S, S_A = np.zeros((nx, np_), dtype=LD), np.zeros((nx, np_)), np.zeros((nx, np_))
    step = max(1, block // (tile * len(X)))
    jobs = []
    for ti, (a0, a1, ac) in enumerate(tiles_of(nx, tile)):
        for tj, (b0, b1, bc) in enumerate(tiles_of(np_, tile)):
            for r0 in range(a0, a1, step):
                jobs.append((slice(r0, min(r0 + step, a1)), slice(b0, b1), x[ac], p[bc], bool(centred[ti, tj])))

    def run(job):
        rows, cols, xc, pc, cen = job
        mu[rows, cols], S[rows, cols], S_A[rows, cols] = _block(hyper, X, w, x, p, rows, cols, xc, pc, cen)

    with ThreadPoolExecutor(threads) as pool:
        list(pool.map(run, jobs))
    tol = 4 * EPS * ((len(X) + 8) * S + S_A) + EPS * float(np.abs(mu).max())
    return mu, tol, centred


def centred_plane(hyper, X, b, x, p, c=1.0, tile=TILE, dtype=np.float64):
    """the same plane by the centred form in EVERY tile, whatever its range, in `dtype` arithmetic: exp(-a c u v) [w e^(x exponent)] [e^(p exponent)]^T,
    and the largest operand exponent met"""
    w = (float(c) * float(hyper[1]) ** 2 * np.asarray(b, dtype=np.float64)).astype(dtype)  # the float64 products the direct sum takes
    out, top = np.zeros((len(x), len(p)), dtype=dtype), -np.inf
    for a0, a1, ac in tiles_of(len(x), tile):
        for b0, b1, bc in tiles_of(len(p), tile):
            ex, ep, cell = split_exponents(hyper, X, x[a0:a1].astype(dtype) - dtype(x[ac]), p[b0:b1].astype(dtype) - dtype(p[bc]), x[ac], p[bc], dtype)
            top = max(top, float(ex.max()), float(ep.max()))
            out[a0:a1, b0:b1] = np.exp(cell) * ((w[None, :] * np.exp(ex)) @ np.exp(ep).T)
    return out, top
