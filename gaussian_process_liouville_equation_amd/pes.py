"""User potentials: a diabatic matrix of your own, tabulated for gple_pes_define (include/gple.h).

    from gaussian_process_liouville_equation_amd import pes
    x_first, dx, V, dV = pes.tabulate(my_surfaces, -16.0, 1.0 / 16, 513)
    model = api.pes_define(2, x_first, dx, V, dV)
    exact.run(api, model=model, ...)

The library evaluates the table as a cubic Hermite interpolant and continues it linearly beyond both ends, so the table has to cover
everything but the asymptotes.
"""
import numpy as np


def tabulate(fun, x_first, dx, n):
    """Tabulate fun(x) -> (V, dV) at the n nodes x_first + dx k: V the symmetric diabatic matrix (num_pes, num_pes) at the scalar x and dV its
    derivative dV/dx.  Returns (x_first, dx, V (n, num_pes, num_pes), dV (n, num_pes, num_pes)), the arguments of Api.pes_define after num_pes.

    Both triangles are made equal (the mean of the two), as gple_pes_define demands exact symmetry.  The nodes are x_first + dx * k in float64,
    the positions the library assigns to them; a dx that is a power of two makes them exact.

    Interpolation error of the table between its ends, for four times differentiable entries: at most dx^4 / 384 * max|V''''| for the values
    and sqrt(3) / 216 * dx^3 * max|V''''| for the derivative (the force), both sharp.  Choose dx from the second."""
    n = int(n)
    if n < 2:
        raise ValueError("a table needs at least two nodes")
    if not (np.isfinite(dx) and dx > 0 and np.isfinite(x_first)):
        raise ValueError("x_first must be finite and dx finite and positive")
    Vs, dVs = [], []
    for k in range(n):
        V, dV = fun(float(x_first) + float(dx) * k)
        V, dV = np.asarray(V, dtype=np.float64), np.asarray(dV, dtype=np.float64)
        if V.ndim != 2 or V.shape[0] != V.shape[1] or dV.shape != V.shape:
            raise ValueError("fun(x) must return two square matrices of the same size")
        if Vs and V.shape != Vs[0].shape:
            raise ValueError("fun(x) must return matrices of one size at every x")
        Vs.append(0.5 * (V + V.T))
        dVs.append(0.5 * (dV + dV.T))
    V, dV = np.stack(Vs), np.stack(dVs)
    if not (np.isfinite(V).all() and np.isfinite(dV).all()):
        raise ValueError("fun(x) must return finite matrices")
    return float(x_first), float(dx), V, dV
