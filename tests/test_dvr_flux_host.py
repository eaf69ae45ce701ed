"""CPU: what the absorber took.  The first half checks the numpy restatement itself (tests/dvr_flux_numpy.py: projectors, the
split of the one-step loss, the recurrence beside the power, against its long-double oracle); those tests use no code of the package and
pass without the feature.  The second half runs the driver, exact.run(boundary=ABSORBING, flux=True), on a numpy stand-in for the api: every
one of those tests fails without the feature."""
import math

import numpy as np
import pytest

from gaussian_process_liouville_equation_amd import exact
from tests import dvr_absorbing_numpy as AN
from tests import dvr_flux_numpy as FN
from tests.test_dvr_absorbing_host import NumpyApi, _packet

EPS = FN.EPS


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_pes, n", AN.SHAPES)
def test_projectors_resolve_the_identity(num_pes, n):
    c = FN.case(num_pes, n)
    P = FN.projectors(c["basis"], c["n_left"])
    assert len(P) == 2 * num_pes and np.abs(sum(P) - np.eye(c["dim"])).max() <= 1e-14
    w = np.diag(np.tile(c["W"], num_pes))
    for p in P:
        assert np.array_equal(p, p.T) or np.abs(p - p.T).max() <= 1e-16
        assert np.abs(p @ p - p).max() <= 1e-14                 # a projector
        assert np.abs(p @ w - w @ p).max() <= 1e-14 * w.max()   # W is one number per grid point: it commutes with every channel


@pytest.mark.parametrize("s", FN.POWERS)
@pytest.mark.parametrize("num_pes, n", AN.SHAPES)
def test_recurrence_against_the_long_double_oracle(num_pes, n, s):
    c = FN.case(num_pes, n)
    U, G = FN.matrices(num_pes, n, s)
    e = FN.e_ref(num_pes, n, s)
    print("flux restatement dim = %d s = %d: e_ref = %.3g, absorbed %.4g of %.3g" % (c["dim"], s, e, c["absorbed"][s].sum(), c["norm2"]))
    assert e <= 1e-12  # measured 5e-16 .. 4.6e-13: the restatement's own rounding over up to 1000 steps at |psi0|^2 = 16
    scale = 8.0 * max(e, EPS * math.sqrt(c["dim"]))
    total = sum(G)
    assert np.abs(total - (np.eye(c["dim"]) - AN.cmul(U.conj(), U))).max() <= scale  # sum_c G_c = I - conj(U) U: the channels miss nothing
    for g in G:
        assert np.array_equal(g, g.conj().T)
    # and on the packet: |psi0|^2 - |U psi0|^2 is what the channels took
    after = U @ c["psi0"]
    assert abs(c["norm2"] - np.vdot(after, after).real - FN.forms(G, c["psi0"]).sum()) <= scale * c["norm2"]


def test_the_packet_leaves_the_short_boxes():
    """at 1000 steps the three short boxes have absorbed 15.1, 8.1 and 3.8 of |psi0|^2 = 16; in the long one the packet has not arrived
    (only its Gaussian tail: less than a millionth)"""
    got = [FN.case(*shape)["absorbed"][1000].sum() for shape in AN.SHAPES]
    assert [round(float(v), 1) for v in got[:3]] == [15.1, 8.1, 3.8] and abs(got[3]) < 1e-6


@pytest.mark.parametrize("num_pes, n", AN.SHAPES)
def test_one_step_is_the_flux_into_the_absorber(num_pes, n):
    """psi^H D_c psi = (2 dt / hbar) <psi| Pi_c W |psi> + O(dt^2): the difference falls to a quarter with every halving of dt (the next term is
    smaller by |H| dt < 0.1 here, so the ratio lies within 0.25 (1 +- 0.3)).  D_c is not positive semidefinite: the packet's own figure on a
    channel it has not reached is slightly negative."""
    c = FN.case(num_pes, n)
    rng = np.random.Generator(np.random.PCG64(7))
    psi = rng.standard_normal(c["dim"]) + 1j * rng.standard_normal(c["dim"])
    w = np.tile(c["W"], num_pes)
    gaps = []
    for halvings in range(3):
        dt = c["dt"] / 2 ** halvings
        D = FN.channels(FN.loss(AN.p4(AN.generator(c["H"], c["W"], num_pes, dt))), c["basis"], c["n_left"])
        textbook = np.array([2.0 * dt / FN.HBAR * np.vdot(psi, FN.project(c["basis"], c["n_left"], ch, (w * psi).real)
                                                        + 1j * FN.project(c["basis"], c["n_left"], ch, (w * psi).imag)).real for ch in range(2 * num_pes)])
        gaps.append(np.abs(FN.forms(D, psi) - textbook).max())
        assert gaps[-1] <= 0.2 * np.abs(textbook).max()
    print("one step dim = %d: gaps %s" % (c["dim"], " ".join("%.3g" % g for g in gaps)))
    for coarse, fine in zip(gaps, gaps[1:]):
        assert 0.25 * 0.7 <= fine / coarse <= 0.25 * 1.3
    _, G = FN.matrices(num_pes, n, 1)
    assert FN.forms(G, c["psi0"]).min() < 0.0


# ---- the driver on a numpy stand-in -------------------------------------------------------------------------------------------------------------
SMALL = dict(AN.SMALL, output_time=64.0)


class FluxApi(NumpyApi):
    """the stand-in of tests/test_dvr_absorbing_host.py with the two new entry points on the restatement"""

    def dvr_flux(self, num_pes, n, H, W, dt, n_steps, basis, n_left, device_out=False, want_u=True):
        self.calls.append(("flux", n_steps, dt, n_left))
        U, G = FN.flux_matrices(H, W, num_pes, dt, n_steps, basis, n_left)
        return (U if want_u else None), np.array(G)

    def dvr_flux_apply(self, num_pes, n, G, psi):
        psi = np.atleast_2d(psi)
        self.calls.append(("flux_apply", len(psi)))
        return np.array([FN.forms(G, v) for v in psi]).reshape(len(psi), 2, num_pes)

    def dvr_propagator(self, *a, **k):
        raise AssertionError("with flux=True the propagator comes from dvr_flux")


def test_flux_run_files_and_records(tmp_path):
    api = FluxApi()
    res = exact.run(api, model=exact.SAC, num_pes=2, boundary=exact.ABSORBING, out_dir=str(tmp_path), write_phase=None, max_outputs=9, chunk_bytes=1_600_000,
                    flux=True, until_absorbed=True, **SMALL)
    s = res["setup"]
    assert [c for c in api.calls if c[0] == "flux"] == [("flux", 512, 0.125, 53)]  # 5 + 48 grid points lie left of the centre x = 0
    assert int(np.sum(s["x"] < 0.0)) == 53 and res["flux_seconds"] > 0.0
    from oracle import evolve_oracle_n as ON
    ref, _ = FN.run_loop(s, 2, exact.SAC, 9, ON.adiabatic(s["x"], exact.SAC, 2)[1])
    # the reference's criteria stop at the sixth output (the packet's <x> passes -x0); this run goes on to max_outputs
    assert len(res["records"]) == len(ref) == 9 and res["stop"] is None
    initial = res["records"][0]["populations"].sum()
    assert not res["records"][0]["absorbed"].any()
    for a, b in zip(res["records"], ref):
        assert a["t"] == b["t"] and a["absorbed"].shape == (2, 2)
        assert np.abs(a["absorbed"] - b["absorbed"]).max() <= 1e-12
        assert abs(a["absorbed"].sum() + a["populations"].sum() - initial) <= 1e-11
    taken = res["records"][-1]["absorbed"]
    assert taken[1].sum() > 0.5 and abs(taken[0]).sum() < 0.01  # by t = 512 most of the packet has left, on the right: transmission
    g = lambda v: float("%g" % v)
    rows = [[float(v) for v in line.split()] for line in open(tmp_path / "absorbed.txt").read().splitlines()]
    assert len(rows) == 9 and all(len(r) == 2 + 2 * 2 for r in rows)
    for row, a in zip(rows, res["records"]):
        assert row == [g(a["t"]), g(a["absorbed"][0, 0]), g(a["absorbed"][0, 1]), g(a["absorbed"][1, 0]), g(a["absorbed"][1, 1]), g(a["populations"].sum())]
    last = res["records"][-1]
    assert np.array_equal(res["absorbed"], last["absorbed"])
    assert res["scattering_line"].split() == res["final_line"].split()[:1] + ["%g" % v for v in last["absorbed"].ravel()] + ["%g" % last["populations"].sum()]
    assert len(open(tmp_path / "averages.txt").read().splitlines()) == 9


def test_until_absorbed_runs_past_the_default_stop_to_the_population_limit():
    """scripted states (as test_every_stop_branch of the sibling file): the reference's criteria stop at the third record ("DIRECTION REVERSED"),
    until_absorbed goes on to the fifth, the first below PplLim, although <x> is negative there"""
    script = [(0.5, 0.9), (0.4, 0.5), (0.3, 2e-4), (-0.2, 5e-5), (0.3, 1e-5)]
    s = exact.setup(boundary=exact.ABSORBING, **SMALL)
    runs = {}
    for until in (False, True):
        said = []
        runs[until] = exact.run(FluxApi([_packet(s, c, w) for c, w in script]), model=exact.SAC, num_pes=2, boundary=exact.ABSORBING, write_phase=None,
                                max_outputs=len(script) + 1, log=said.append, flux=True, until_absorbed=until, **SMALL)
        assert said[-1] == runs[until]["stop"]
    assert len(runs[False]["records"]) == 3 and runs[False]["stop"].startswith("DIRECTION REVERSED")
    assert len(runs[True]["records"]) == 5 and runs[True]["records"][-1]["x"] < 0.0
    assert runs[True]["stop"] == "ALMOST ALL POPULATION HAVE BEEN ABSORBED, STOP EVOLVING AT %g" % runs[True]["stop_time"]
    # max_outputs still ends a run that never gets there
    short = exact.run(NumpyApi([_packet(s, c, w) for c, w in script]), model=exact.SAC, num_pes=2, boundary=exact.ABSORBING, write_phase=None, max_outputs=3,
                      until_absorbed=True, **SMALL)
    assert len(short["records"]) == 3 and short["stop"] is None and "absorbed" not in short


def test_flux_belongs_to_the_absorbing_boundary():
    for kw in (dict(flux=True), dict(until_absorbed=True), dict(flux=True, boundary=exact.REFLECTIVE)):
        with pytest.raises(ValueError):
            exact.run(FluxApi(), model=exact.SAC, num_pes=2, write_phase=None, max_outputs=1, **{**SMALL, **kw})


def test_without_the_keywords_nothing_changes(tmp_path):
    """both keywords false: the files, the records and the returned keys of a call that does not know them"""
    outs = []
    for k, kw in enumerate((dict(), dict(flux=False, until_absorbed=False))):
        d = tmp_path / str(k)
        res = exact.run(NumpyApi(), model=exact.SAC, num_pes=2, boundary=exact.ABSORBING, out_dir=str(d), write_phase="text", max_outputs=4,
                        chunk_bytes=1_600_000, **SMALL, **kw)
        outs.append((res, {p.name: p.read_bytes() for p in sorted(d.iterdir())}))
    (a, fa), (b, fb) = outs
    assert fa == fb and sorted(fa) == ["averages.txt", "p.txt", "phase.txt", "psi.txt", "t.txt", "x.txt"]
    assert sorted(a) == sorted(b) and "absorbed" not in a and "scattering_line" not in a
    assert a["final_line"] == b["final_line"] and a["stop"] == b["stop"] and len(a["records"]) == len(b["records"]) == 4
    for ra, rb in zip(a["records"], b["records"]):
        assert sorted(ra) == sorted(rb) == ["E", "p", "phase_averages", "populations", "t", "x"]
        assert all(np.array_equal(ra[k], rb[k]) for k in ra)
