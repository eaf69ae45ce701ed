"""The closed-form potentials the scattering tests share (tests/test_scatter_host.py, tests/test_gpu_scatter.py): functions x (m,) -> (V, dV / dx)
in x's dtype, the interface of tests/scatter_numpy.march (which reads V alone) and, through scalar(), of pes.tabulate."""
import numpy as np

MASS, P_IN = 2000.0, 6.5
E_IN = P_IN * P_IN / 2.0 / MASS
BOX = 20.0
ANGLE = 0.6


def _sech2(x, a):
    """sech^2(a x) and its x derivative"""
    s = 1.0 / np.cosh(a * x) ** 2
    return s, -2.0 * a * s * np.tanh(a * x)


def eckart(x):
    """level 0: the Eckart barrier 0.01 sech^2(x); level 1, decoupled: 0.003 + 0.005 sech^2(x)"""
    V, dV = np.zeros(x.shape + (2, 2), dtype=x.dtype), np.zeros(x.shape + (2, 2), dtype=x.dtype)
    s, ds = _sech2(x, 1.0)
    V[:, 0, 0], dV[:, 0, 0] = 0.01 * s, 0.01 * ds
    V[:, 1, 1], dV[:, 1, 1] = 0.003 + 0.005 * s, 0.005 * ds
    return V, dV


def rotated(x):
    """U diag(0.01 sech^2 x, 0.004 + 0.006 sech^2(1.5 x)) U^T with the constant rotation U of angle 0.6: two adiabatic channels that never mix"""
    ty = x.dtype.type
    c, s = np.cos(ty(ANGLE)), np.sin(ty(ANGLE))
    U = np.array([[c, -s], [s, c]], dtype=x.dtype)
    a, da = _sech2(x, 1.0)
    b, db = _sech2(x, 1.5)
    D, dD = np.zeros(x.shape + (2, 2), dtype=x.dtype), np.zeros(x.shape + (2, 2), dtype=x.dtype)
    D[:, 0, 0], dD[:, 0, 0] = 0.01 * a, 0.01 * da
    D[:, 1, 1], dD[:, 1, 1] = 0.004 + 0.006 * b, 0.006 * db
    V, dV = U @ D @ U.T, U @ dD @ U.T
    return 0.5 * (V + np.swapaxes(V, 1, 2)), 0.5 * (dV + np.swapaxes(dV, 1, 2))


def closed_forms():
    """the transmission of each closed-form case per adiabatic channel at E_IN, long double: eckart's level 0, and both channels of rotated"""
    from tests import scatter_numpy as SN
    k0 = np.sqrt(np.longdouble(2) * MASS * np.longdouble(E_IN))
    k1 = np.sqrt(np.longdouble(2) * MASS * (np.longdouble(E_IN) - np.longdouble(0.004)))
    return dict(eckart=SN.eckart_transmission(k0, 0.01, 1.0, MASS), rotated=(SN.eckart_transmission(k0, 0.01, 1.0, MASS), SN.eckart_transmission(k1, 0.006, 1.5, MASS)))


def scalar(potential):
    """fun(x) -> (V, dV / dx) at a scalar x, the argument of pes.tabulate"""
    def fun(x):
        V, dV = potential(np.array([x], dtype=np.float64))
        return V[0], dV[0]
    return fun
