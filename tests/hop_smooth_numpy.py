"""numpy restatement of gple_hop_smooth / gple_hop_smooth_mf (csrc/gple_hop.hip, include/gple.h, DESIGN.md §17 "The ensemble in phase space,
smoothed"), written from the definition in the header on the amplitudes of tests/hop_density_numpy.py, generic in dtype: float64, and
numpy.longdouble with its complex type.

    selection(state, mean_field, bin_all)   who is used, who is selected but not finite
    terms(potential, state, ...)            x, p and the N^2 real weights u_q of the used trajectories, and the tallies (used, nonfinite)
    smooth(potential, state, grid, h, n_norm, mean_field, bin_all, dtype, with_bound)
                                            rho (N, N, n_x, n_p) complex, the tallies and, with_bound, B (N, N, n_x, n_p, 2) real, the bound
                                            of the real and of the imaginary part: the plain sum in index order, one trajectory after the other
    NumpyHopSmoothApi                       the numpy api of tests/hop_density_mf_numpy.py (which has the calls of tests/hop_density_numpy.py too)
                                            with hop_smooth / hop_smooth_mf, for hopping.run(phase_smooth=...); every call is recorded

The bound of a float64 evaluation of an entry against the exact value, eps = 2^-52 (numpy's float64 epsilon):
    B = eps s sum_i g_x g_p (|u_i| (n_used + 2 t_x^2 + 2 t_p^2 + 4 |t_x| (|x_k| + |x_i|) / h_x + 4 |t_p| (|p_j| + |p_i|) / h_p) + 16 m_i)
n_used: any summation order; 2 t^2: the rounding of the exponent and of exp, scaled by the argument; the last two: the rounding of x_k and of
the difference; 16: the remaining products, the weight's own among them.  m_i is what those last roundings are relative to.  For a count plane
(u = 0 or 1, exact) it is |u_i|.  For a weight formed from the amplitudes it is |c_i|^2 = sum_k |c_k|^2 (1 for a unit vector), not |u_i|:
c = C^T b is rounded relative to |b|, so re = cre_a cre_b + cim_a cim_b carries an absolute error of a few eps |c|^2 however small the sum
itself comes out.  Found on the first case tried (DAC, p0 = 10, 24 x 40): one trajectory with re = -3.5e-4 from terms of size 0.25 dominates a
cell, its float64 weight differs from the long double one by 9e-17 (7.5e-14 of itself), and with |u_i| in that place the float64 restatement
misses the bound by a factor 2.2.  With |c_i|^2 >= |u_i| the bound is never below the one with |u_i| throughout.  For a lower plane B is that
of its upper one.  The error of a float64 field against the long double one is held
against B of the long double evaluation.
B is relative to the terms, so it says nothing where float64 underflows: at t = 40 a Gaussian is below 2^-1074 and the float64 term is 0,
while long double still holds it (every grid of 64 lines with h = 0.3 d has such entries).  There the absolute error of gradual underflow
applies: a Gaussian, the two products of a term and its addition each lose at most the spacing of the subnormals, 2^-1074, the factors beside
them being at most 1, and so does the product with s.  B therefore carries the absolute term UNDERFLOW = 2^-1074 (4 s n_used + 1), about
1e-320, on every entry that has a bound at all.

grid is the 6-tuple (x_first, dx, n_x, p_first, dp, n_p), h the pair (h_x, h_p)."""
import numpy as np

from tests import hop_density_mf_numpy as HDM
from tests import hop_density_numpy as HD

EPS = float(np.finfo(np.float64).eps)
SUBNORMAL = np.longdouble(2.0) ** -1074  # the spacing of float64 below 2^-1022


def selection(state, mean_field=False, bin_all=False):
    """(used, nonfinite) bool (n,): the selection of the bin call of the same form; a selected trajectory is used when x and p are finite"""
    x, p, b, surface, status = state
    N = np.asarray(b).shape[1]
    status = np.asarray(status)
    selected = (status >= 0) & (status <= 2) & ((status == 0) | bool(bin_all))
    if not mean_field:
        surface = np.asarray(surface)
        selected &= (surface >= 0) & (surface < N)
    finite = np.isfinite(np.asarray(x, dtype=np.float64)) & np.isfinite(np.asarray(p, dtype=np.float64))
    return selected & finite, selected & ~finite


def terms(potential, state, mean_field=False, bin_all=False, dtype=np.float64):
    """x (m,), p (m,), u (N^2, m), m (N^2, m) of the m used trajectories in index order, and (used, nonfinite).  u: the diagonal
    a = 0 ... N - 1, then (re, im) per pair a < b in row-major order; m: what the rounding of u is relative to (the module's text)"""
    used, nonfinite = selection(state, mean_field, bin_all)
    N = np.asarray(state[2]).shape[1]
    sub = tuple(np.asarray(v)[used] for v in state)
    x, p = sub[0].astype(dtype), sub[1].astype(dtype)
    u = np.zeros((N * N, int(used.sum())), dtype=dtype)
    m = np.zeros_like(u)
    if used.any():
        c = HD.amplitudes(potential, (x, p, sub[2].astype(np.result_type(dtype, np.complex64)), sub[3], sub[4]))
        cre, cim = c.real.astype(dtype), c.imag.astype(dtype)
        for a in range(N):
            u[a] = cre[:, a] * cre[:, a] + cim[:, a] * cim[:, a] if mean_field else (sub[3] == a).astype(dtype)
        q = N
        for a in range(N):
            for b in range(a + 1, N):
                u[q] = cre[:, a] * cre[:, b] + cim[:, a] * cim[:, b]
                u[q + 1] = cim[:, a] * cre[:, b] - cre[:, a] * cim[:, b]
                q += 2
        m[:] = (cre * cre + cim * cim).sum(axis=1)[None, :]
        if not mean_field:
            m[:N] = u[:N]
    return x, p, u, m, (int(used.sum()), int(nonfinite.sum()))


def scale(n_norm, h, dtype=np.float64):
    """s = 1 / ((double)n_norm 2 pi h_x h_p), the denominator left to right"""
    ty = np.dtype(dtype).type
    return ty(1) / (ty(n_norm) * (ty(8) * np.arctan(ty(1))) * ty(h[0]) * ty(h[1]))


def smooth(potential, state, grid, h, n_norm, mean_field=False, bin_all=False, dtype=np.float64, with_bound=False):
    """gple_hop_smooth (mean_field: gple_hop_smooth_mf) -> rho, (used, nonfinite) [, B]"""
    ty = np.dtype(dtype).type
    x_first, dx, n_x, p_first, dp, n_p = grid
    n_x, n_p = int(n_x), int(n_p)
    N = np.asarray(state[2]).shape[1]
    x, p, u, m, tallies = terms(potential, state, mean_field, bin_all, dtype)
    xk = ty(x_first) + ty(dx) * np.arange(n_x).astype(dtype)
    pj = ty(p_first) + ty(dp) * np.arange(n_p).astype(dtype)
    h_x, h_p = ty(h[0]), ty(h[1])
    s = scale(n_norm, h, dtype)
    total = np.zeros((N * N, n_x, n_p), dtype=dtype)
    bound = np.zeros((N * N, n_x, n_p), dtype=dtype)
    with np.errstate(under="ignore", over="ignore"):
        for i in range(len(x)):  # the plain sum, in index order
            t_x, t_p = (xk - x[i]) / h_x, (pj - p[i]) / h_p
            total += u[:, i, None, None] * np.outer(np.exp(ty(-0.5) * t_x * t_x), np.exp(ty(-0.5) * t_p * t_p))[None]
        if with_bound and len(x):
            # B's sum as three products over the trajectory index: |u| n_used + 16 m, plus a part that depends on (k, i) alone, plus one
            # that depends on (i, j) alone.  A Gaussian that is exactly 0 has no error (and its factor may be infinite)
            t_x, t_p = (xk[:, None] - x[None, :]) / h_x, (pj[None, :] - p[:, None]) / h_p
            g_x, g_p = np.exp(ty(-0.5) * t_x * t_x), np.exp(ty(-0.5) * t_p * t_p)
            with np.errstate(invalid="ignore"):
                w_x = np.where(g_x > 0, ty(2) * t_x * t_x + ty(4) * np.abs(t_x) * (np.abs(xk)[:, None] + np.abs(x)[None, :]) / h_x, ty(0))
                w_p = np.where(g_p > 0, ty(2) * t_p * t_p + ty(4) * np.abs(t_p) * (np.abs(pj)[None, :] + np.abs(p)[:, None]) / h_p, ty(0))
            for q in range(N * N):
                a_x = g_x * np.abs(u[q])[None, :]
                flat = g_x * (ty(tallies[0]) * np.abs(u[q]) + ty(16) * m[q])[None, :]
                bound[q] = flat @ g_p + (a_x * w_x) @ g_p + a_x @ (w_p * g_p)
            under = (np.longdouble(s) * SUBNORMAL * (4 * tallies[0]) + SUBNORMAL).astype(dtype) / (ty(EPS) * s)  # UNDERFLOW, scaled as the sum is below
            bound = np.where(bound > 0, bound + under, bound)
    rho = np.zeros((N, N, n_x, n_p), dtype=np.result_type(dtype, np.complex64))
    B = np.zeros((N, N, n_x, n_p, 2), dtype=dtype)  # per (re, im) part; Im rho_aa is +0 exactly: its bound is 0
    for a in range(N):
        rho[a, a].real = s * total[a]  # the imaginary part stays +0
        B[a, a, :, :, 0] = ty(EPS) * s * bound[a]
    q = N
    for a in range(N):
        for b in range(a + 1, N):
            rho[a, b].real = rho[b, a].real = s * total[q]
            rho[a, b].imag = s * total[q + 1]
            rho[b, a].imag = s * (ty(0) - total[q + 1])  # from the negated sum: +0 where the sum is 0
            B[a, b, :, :, 0] = B[b, a, :, :, 0] = ty(EPS) * s * bound[q]
            B[a, b, :, :, 1] = B[b, a, :, :, 1] = ty(EPS) * s * bound[q + 1]
            q += 2
    if with_bound:
        return rho, tallies, B
    return rho, tallies


class NumpyHopSmoothApi(HDM.NumpyHopDensityMfApi):
    """the numpy api of hopping.run(phase_grid=..., phase_density=...) with the two smoothed densities"""

    def hop_smooth(self, num_pes, model, state, grid, bandwidth, n_norm, bin_all=False):
        self.calls.append(("smooth",))
        return smooth(self._potential(num_pes, model), self._narrow(state), grid, bandwidth, n_norm, False, bin_all)

    def hop_smooth_mf(self, num_pes, model, state, grid, bandwidth, n_norm, bin_all=False):
        self.calls.append(("smooth_mf",))
        return smooth(self._potential(num_pes, model), self._narrow(state), grid, bandwidth, n_norm, True, bin_all)
