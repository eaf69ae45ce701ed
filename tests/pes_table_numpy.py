"""float64 restatement of the tabulated potential of gple_pes_define (include/gple.h; csrc/gple_pes_n.h, table_diabatic_n), in the header's
operation order, and a generic adiabatic (eigh with the library's sign convention) for it.  install() makes the restatements that take their
potentials from oracle/evolve_oracle_n.py (tests/dvr_numpy.py, tests/mqcl_numpy.py, the N-level tick's oracle) see tables under chosen ids."""
import numpy as np

from oracle import evolve_oracle_n as ON

EPS = np.finfo(np.float64).eps
DAC_A, DAC_B, DAC_C, DAC_D, DAC_E = 0.10, 0.28, 0.015, 0.06, 0.05  # Tully's dual avoided crossing (pes.cpp)
DAC_F4 = max(12 * DAC_A * DAC_B ** 2, 12 * DAC_C * DAC_D ** 2)     # max |d^4/dx^4| of its entries (a Gaussian's fourth derivative peaks at 0)


class Table:
    """V, dV (n, N, N) at x_first + dx k; m = dx dV is formed once, as the library does when the model is defined"""

    def __init__(self, x_first, dx, V, dV):
        self.x_first, self.dx = float(x_first), float(dx)
        self.V, self.dV = np.array(V, dtype=np.float64), np.array(dV, dtype=np.float64)
        self.m = self.dx * self.dV
        self.n, self.num_pes = self.V.shape[0], self.V.shape[1]

    def args(self):
        return self.x_first, self.dx, self.V, self.dV

    def nodes(self):
        return self.x_first + self.dx * np.arange(self.n)

    def locate(self, x):
        """(s, k, t, left, right) of the header: left / right mark the linear continuation"""
        s = (x - self.x_first) / self.dx
        k = np.clip(np.floor(s), 0, self.n - 2).astype(np.int64)
        return s, k, s - k, s < 0, s > self.n - 1

    def diabatic(self, x):
        """(V (M, N, N), F = -V' (M, N, N)) at x (M,)"""
        x = np.asarray(x, dtype=np.float64).reshape(-1)
        s, k, t, left, right = self.locate(x)
        t = t[:, None, None]
        v0, v1, m0, m1 = self.V[k], self.V[k + 1], self.m[k], self.m[k + 1]
        delta = v1 - v0
        c2 = 3.0 * delta - (2.0 * m0 + m1)
        c3 = (m0 + m1) - 2.0 * delta
        V = v0 + t * (m0 + t * (c2 + t * c3))
        dV = (m0 + t * (2.0 * c2 + 3.0 * t * c3)) / self.dx
        for mask, node in ((left, 0), (right, self.n - 1)):
            if mask.any():
                h = (x[mask] - (self.x_first + self.dx * node))[:, None, None]
                V[mask] = self.V[node] + self.dV[node] * h
                dV[mask] = self.dV[node]
        return V, -dV

    def tolerance(self, x):
        """the entrywise bound of the device's value against this restatement (the two differ through fma contraction only):
        64 eps (|V_k| + |V_k+1| + |m_k| + |m_k+1|); the derivative's is this over dx"""
        _, k, _, _, _ = self.locate(np.asarray(x, dtype=np.float64).reshape(-1))
        return 64 * EPS * (np.abs(self.V[k]) + np.abs(self.V[k + 1]) + np.abs(self.m[k]) + np.abs(self.m[k + 1]))


def adiabatic_of(V, Fd):
    """E ascending, C (columns, last non-zero component positive), F = C^T Fd C symmetrised, NAC[j, k] = F[j, k] / (E_j - E_k): what
    oracle/evolve_oracle_n.adiabatic forms for a genuinely coupled model"""
    num_pes = V.shape[1]
    E, C = np.linalg.eigh(V)
    for m in range(len(E)):
        for k in range(num_pes):
            nz = np.nonzero(C[m, :, k] != 0.0)[0]
            if len(nz) and C[m, nz[-1], k] < 0:
                C[m, :, k] = -C[m, :, k]
    F = np.einsum("mak,mab,mbl->mkl", C, Fd, C)
    F = 0.5 * (F + np.swapaxes(F, 1, 2))
    NAC = np.zeros_like(F)
    for j in range(1, num_pes):
        for k in range(j):
            with np.errstate(divide="ignore", invalid="ignore"):
                d = np.where(F[:, j, k] == 0.0, 0.0, F[:, j, k] / (E[:, j] - E[:, k]))
            NAC[:, j, k], NAC[:, k, j] = d, -d
    return E, C, F, NAC


def install(monkeypatch, tables):
    """tables: {model id: Table}.  ON.diabatic and ON.adiabatic answer from the table for these ids (both are patched: ON.adiabatic treats every
    three-level model but TSAC as Tully's two surfaces plus a spectator) and as before for every other id"""
    diabatic, adiabatic = ON.diabatic, ON.adiabatic

    def patched_diabatic(x, model, num_pes):
        if model in tables:
            assert tables[model].num_pes == num_pes
            return tables[model].diabatic(x)
        return diabatic(x, model, num_pes)

    def patched_adiabatic(x, model, num_pes):
        if model in tables:
            return adiabatic_of(*patched_diabatic(x, model, num_pes))
        return adiabatic(x, model, num_pes)

    monkeypatch.setattr(ON, "diabatic", patched_diabatic)
    monkeypatch.setattr(ON, "adiabatic", patched_adiabatic)


def dac(x):
    """Tully's DAC at scalar or array x: (V (..., 2, 2), dV/dx (..., 2, 2)), analytic"""
    x = np.asarray(x, dtype=np.float64)
    V, dV = np.zeros(x.shape + (2, 2)), np.zeros(x.shape + (2, 2))
    V[..., 1, 1] = DAC_E - DAC_A * np.exp(-DAC_B * x * x)
    V[..., 0, 1] = V[..., 1, 0] = DAC_C * np.exp(-DAC_D * x * x)
    dV[..., 1, 1] = 2 * DAC_A * DAC_B * x * np.exp(-DAC_B * x * x)
    dV[..., 0, 1] = dV[..., 1, 0] = -2 * DAC_C * DAC_D * x * np.exp(-DAC_D * x * x)
    return V, dV


def dac_table(dx, lo=-16.0, hi=16.0):
    n = int(round((hi - lo) / dx)) + 1
    return Table(lo, dx, *dac(lo + dx * np.arange(n)))


def other_dac(x):
    """a dual avoided crossing with constants of its own (not in the library): two levels"""
    x = np.asarray(x, dtype=np.float64)
    A, B, C, D, E = 0.08, 0.35, 0.012, 0.09, 0.04
    V, dV = np.zeros(x.shape + (2, 2)), np.zeros(x.shape + (2, 2))
    V[..., 0, 0], dV[..., 0, 0] = 0.002 * np.tanh(0.5 * x), 0.001 / np.cosh(0.5 * x) ** 2
    V[..., 1, 1] = E - A * np.exp(-B * x * x)
    V[..., 0, 1] = V[..., 1, 0] = C * np.exp(-D * x * x)
    dV[..., 1, 1] = 2 * A * B * x * np.exp(-B * x * x)
    dV[..., 0, 1] = dV[..., 1, 0] = -2 * C * D * x * np.exp(-D * x * x)
    return V, dV


def three_level(x):
    """a variation on TSAC: three coupled levels, every coupling non-zero and the middle level tilted"""
    x = np.asarray(x, dtype=np.float64)
    A, B, C, D = 0.03, 0.6, 0.006, 0.4
    t, g, th = np.tanh(B * x), 1.0 / np.cosh(D * x), np.tanh(D * x)
    V, dV = np.zeros(x.shape + (3, 3)), np.zeros(x.shape + (3, 3))
    V[..., 0, 0], V[..., 1, 1], V[..., 2, 2] = A * t, 0.004 * np.exp(-0.2 * x * x), -A * t
    dV[..., 0, 0], dV[..., 1, 1], dV[..., 2, 2] = A * B * (1 - t * t), -0.0016 * x * np.exp(-0.2 * x * x), -A * B * (1 - t * t)
    for (i, j, c) in ((0, 1, C), (1, 2, 1.5 * C), (0, 2, 0.3 * C)):
        V[..., i, j] = V[..., j, i] = c * g
        dV[..., i, j] = dV[..., j, i] = -c * D * g * th
    return V, dV


def function_table(fun, lo, hi, dx):
    n = int(round((hi - lo) / dx)) + 1
    return Table(lo, dx, *fun(lo + dx * np.arange(n)))


def random_table(num_pes, n, rng, x_first=-1.25, dx=0.375):
    """random smooth entries: a few low harmonics per entry with random amplitudes and phases, derivative analytic"""
    x = x_first + dx * np.arange(n)
    V, dV = np.zeros((n, num_pes, num_pes)), np.zeros((n, num_pes, num_pes))
    for i in range(num_pes):
        for j in range(i + 1):
            for w in (0.3, 0.7, 1.1):
                a, ph = rng.normal() * 0.02, rng.uniform(0, 2 * np.pi)
                V[:, i, j] += a * np.sin(w * x + ph)
                dV[:, i, j] += a * w * np.cos(w * x + ph)
            V[:, j, i], dV[:, j, i] = V[:, i, j], dV[:, i, j]
    return Table(x_first, dx, V, dV)
