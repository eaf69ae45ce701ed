"""CPU: the binding of gple_nlml_batch / gple_nlml_fit_planes, the fit= choice of the reconstruction driver on a recording Api (which entry
points it reaches, with which planes), and the resource budget of nlml_batch_kernel from the cross-compiled ISA."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from gaussian_process_liouville_equation_amd import _capi, reconstruct as R
from tests.conftest import ROOT
from tests.test_recon_cross_host import RecordingApi

CSRC = os.path.join(ROOT, "gaussian_process_liouville_equation_amd", "csrc")


def test_binding_declares_the_batched_entry_points():
    assert "nlml_batch" in _capi.GPLE_SYMBOLS and "nlml_fit_planes" in _capi.GPLE_SYMBOLS
    assert [n for n, _ in _capi.NlmlProblem._fields_] == ["x", "X", "y", "N"] and _capi.NlmlProblem.x.size == 40
    assert [n for n, _ in _capi.NlmlFitPlane._fields_] == ["X", "y", "N", "start", "lb", "ub"]
    assert _capi.NlmlFitPlane.start.size == _capi.NlmlFitPlane.lb.size == _capi.NlmlFitPlane.ub.size == 40
    assert C.sizeof(_capi.NlmlProblem) == 64 and C.sizeof(_capi.NlmlFitPlane) == 144
    assert _capi.NLML_BATCH_MAX_N == 256
    assert callable(_capi.Api.nlml_batch) and callable(_capi.Api.nlml_fit_planes) and callable(R.optimize_planes)
    header = open(os.path.join(ROOT, "include", "gple.h")).read()
    assert "#define GPLE_NLML_BATCH_MAX_N 256" in header


class FitRecordingApi(RecordingApi):
    """RecordingApi with gple_nlml_fit_planes; plane 1 is 0 everywhere (no fit), and `sizes` overrides the number of selected points per plane"""

    def __init__(self, nx, np_, sizes=None):
        super().__init__(nx, np_)
        self.sizes, self.fits, self.lib = sizes or {}, [], None

    def grid_survey(self, *args):
        s = super().grid_survey(*args)
        s[1, 0], s[1, 1] = 0.005, -0.005
        return s

    def grid_select(self, num_pes, rho, x, p, q, n, seed, uniform=False):
        return super().grid_select(num_pes, rho, x, p, q, self.sizes.get(q, n), seed, uniform)

    def _recon(self, name, width, planes, want_pred):
        assert planes[1] is None
        return super()._recon(name, width, [pl for pl in planes if pl is not None], want_pred)

    def nlml_fit_planes(self, planes, cross=False, options=None, want_weights=False):
        self.calls.append(("nlml_fit_planes", 5 if cross else 4))
        self.fits.append((planes, cross, options, want_weights))
        P = len(planes)
        return (np.array([np.clip(pl[2], pl[3], pl[4]) for pl in planes]), np.arange(1.0, P + 1), np.full(P, 7, dtype=np.int32),
                [np.full(len(pl[1]), 0.02) for pl in planes])


def stub_searches(monkeypatch):
    ends = lambda lib, f, start, lower, upper, options=None: (list(np.clip(start, lower, upper)), f(list(start)), 1)
    monkeypatch.setattr(_capi, "minimize_neldermead", ends)
    monkeypatch.setattr(_capi, "minimize_auglag_eq", lambda lib, f, con, m, start, lower, upper, options=None: (list(start), f(list(start), True)[0], 1))


def run(api, nx=12, np_=9, **kw):
    x, p = np.linspace(-3.0, 3.0, nx), np.linspace(10.0, 20.0, np_)
    return R.reconstruct(api, R.State(api, 2, 1, x, p, 2000.0), np.zeros((2, 2, nx, np_), dtype=complex), n_points=6, **kw)


@pytest.mark.parametrize("kernel, width", [("nocross", 4), ("cross", 5)])
def test_batched_fit_is_one_call_with_the_live_planes(monkeypatch, kernel, width):
    stub_searches(monkeypatch)
    api = FitRecordingApi(12, 9)
    rec = run(api, fit="batched", kernel=kernel, maxeval=40)
    names = [n for n, _ in api.calls]
    assert names.count("nlml_fit_planes") == 1 and "nlml" not in names and not any(n.endswith("weights") for n in names)
    planes, cross, options, want_weights = api.fits[0]
    assert len(planes) == 3 and cross == (width == 5) and want_weights and options.max_eval == 40 and options.xtol_abs == R.XTOL_ABS
    _, _, first = R.set_initial_value(api.grid_survey(2, 1, None, None, None, 2000.0, 0.5, 1.1), np.linspace(-3.0, 3.0, 12), np.linspace(10.0, 20.0, 9), 2, kernel)
    for pl, q in zip(planes, (0, 2, 3)):  # plane 1 is 0 everywhere: not fitted, its hyper-parameters stay
        X, y = api.grid_select(2, None, None, None, q, 6, 0)[1:3]
        assert np.array_equal(pl[0], X) and np.array_equal(pl[1], y) and np.array_equal(pl[2], first[q])
    assert rec["is_small"].tolist() == [False, True, False, False] and np.array_equal(rec["hyper"][1], first[1])
    assert rec["nlml"] == 1.0 + 2.0 + 3.0 and rec["evaluations"] == 21 and rec["hyper"].shape == (4, width)


def test_serial_fit_and_the_default_make_the_calls_of_before(monkeypatch):
    stub_searches(monkeypatch)
    assert inspect.signature(R.reconstruct).parameters["fit"].default == "serial"
    assert inspect.signature(R.run_mqcl).parameters["fit"].default == "serial"
    expected = [("nlml", 4)] * 9 + [("nlml_weights", 4)] * 3 + [("grid_reconstruct", 4)] * 2  # per live plane: both searches' call and the value at the result
    records = []
    for kw in ({}, {"fit": "serial"}):
        api = FitRecordingApi(12, 9)
        records.append(run(api, **kw))
        assert api.calls == expected and not api.fits
    assert np.array_equal(records[0]["hyper"], records[1]["hyper"]) and records[0]["nlml"] == records[1]["nlml"]
    with pytest.raises(ValueError):
        run(FitRecordingApi(12, 9), fit="both")


def test_a_plane_above_the_limit_falls_back_to_optimize(monkeypatch):
    stub_searches(monkeypatch)
    api = FitRecordingApi(12, 9, sizes={2: 300})
    rec = run(api, fit="batched")
    planes = api.fits[0][0]
    assert len(api.fits) == 1 and [len(pl[1]) for pl in planes] == [6, 6]  # planes 0 and 3
    assert api.calls.count(("nlml", 4)) == 3 and api.calls.count(("nlml_weights", 4)) == 1  # plane 2: optimize, then its weights
    assert len(rec["features"][2]) == 300 and rec["evaluations"] == 7 + 7 + 3


@pytest.fixture(scope="module")
def batch_asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "gple_nlml_batch.s"
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++20", "--offload-arch=gfx950", "--cuda-device-only", "-S", f"-I{os.path.join(ROOT, 'include')}",
                    os.path.join(CSRC, "gple_nlml_batch.hip"), "-o", str(out)], check=True, capture_output=True)
    text = out.read_text()
    return {m.group(1): m.group(0) for m in re.finditer(r"^(_ZN4gple\S+):.*?\.end_amdhsa_kernel", text, flags=re.S | re.M)}


def test_the_batch_kernel_stays_inside_its_budget(batch_asm):
    """no scratch, at most 64 KB of LDS (two workgroups share a compute unit), the products on the fp64 MFMA with the accumulators inside the
    register budget of two waves per SIMD, and no floating-point atomics"""
    bodies = [body for name, body in batch_asm.items() if "nlml_batch_kernel" in name]
    assert len(bodies) == 1
    body = bodies[0]
    assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", body)
    assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body).group(1)) <= 65536
    assert "v_mfma_f64_16x16x4_f64" in body or "v_mfma_f64_16x16x4f64" in body
    assert int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1)) <= 256
    assert not re.search(r"atomic_(add|min|max|pk_add)_f", body)
