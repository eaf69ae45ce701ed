"""CPU: hopping.run and hopping.scan are one loop each over the table of methods (hopping.TABLE).  What a merged loop could smooth over by
accident is pinned here per method on the numpy stand-ins: the keys of the results and of the records, with the asymmetries between the
methods that tests and examples read, the literal sequence of api calls, and that nothing but the table and _method knows a method by name."""
import ast
import inspect

import numpy as np
import pytest

from gaussian_process_liouville_equation_amd import hopping
from tests import hop_mash_numpy as HA
from tests import hop_mf_numpy as HM
from tests import hop_numpy as HN
from tests import hop_scan_numpy as HS
from tests import hop_sqc_numpy as HQ
from tests.test_hop_mash_host import RUN, SCAN  # 48 trajectories; 3 groups of 12

NAMES = ("fssh", "ehrenfest", "sqc", "mash")
APIS = {"fssh": HS.NumpyScanApi, "ehrenfest": HM.NumpyMfApi, "sqc": HQ.NumpySqcApi, "mash": HA.NumpyMashApi}
UNPACKED = {"fssh": hopping.unpack(np.zeros(11), 2, 1), "ehrenfest": hopping.unpack_mf(np.zeros(12), 2, 1), "sqc": hopping.unpack_sqc(np.zeros(17), 2, 1, 0.0),
            "mash": hopping.unpack(np.zeros(11), 2, 1)}
RUN_KEYS = {"setup", "dt", "output_step", "total_step", "n_traj", "records", "stop", "state", "scattered", "scattering_line", "stop_time", "steps", "total_seconds",
            "decoherence", "edc_c", "method", "phase_density"}
SCAN_KEYS = {"setups", "dt", "n_per_group", "total_step", "max_steps", "steps", "stop", "state", "hop_counts", "rows", "head", "scattered", "running", "stderr", "hops",
             "frustrated", "energy_drift", "lines", "total_seconds", "decoherence", "edc_c", "method"}
SQC_KEYS = {"window", "gamma", "n_finished_windowed", "unassigned_finished"}
WIDTH = {"fssh": 4 * 2 + 3, "ehrenfest": 3 * 2 + 6, "sqc": 4 * 2 + 9, "mash": 4 * 2 + 3}  # the sums of an observe at two levels
THIRD = 1.0 / 3.0  # the customary gamma of the triangle window, whose code is 1


@pytest.fixture(scope="module")
def ran():
    """per method (the api, the result) of run(max_outputs=3) and of scan(chunk_steps=128, max_steps=256) with groups of 4"""
    out = {}
    for name in NAMES:
        a, b = APIS[name](), APIS[name]()
        out[name] = ((a, hopping.run(a, method=name, max_outputs=3, **RUN)),
                     (b, hopping.scan(b, method=name, fixed=False, chunk_steps=128, max_steps=256, **dict(SCAN, n_per_group=4))))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_the_results_and_the_records_have_the_keys_of_their_method(ran, name):
    (_, run), (_, scan) = ran[name]
    sqc = name == "sqc"
    assert set(run) == (RUN_KEYS - {"phase_density"} | SQC_KEYS if sqc else RUN_KEYS)
    assert set(scan) == (SCAN_KEYS | SQC_KEYS if sqc else SCAN_KEYS)
    assert len(run["records"]) == 3 and all(set(rec) == set(UNPACKED[name]) | {"t"} for rec in run["records"])
    for res in (run, scan):
        assert res["method"] == name and res["decoherence"] is None and res["edc_c"] == (None if sqc else 0.1)
        if sqc:  # the window as its code, the customary gamma
            assert res["window"] == 1 and res["gamma"] == THIRD
    assert "phase_density" in run or sqc
    assert run["scattered"].shape == (2, 2) and scan["scattered"].shape == (3, 2, 2) and scan["rows"].shape == (3, WIDTH[name])
    if name in ("fssh", "mash"):  # the two whose grouped step counts its hops
        assert scan["hop_counts"].shape == (12, 2) and scan["hop_counts"].dtype == np.int32
    else:
        assert scan["hop_counts"] is None and not scan["hops"].any() and not scan["frustrated"].any()
    if sqc:  # numbers from run(), a row per group from scan()
        assert isinstance(run["n_finished_windowed"], float) and isinstance(run["unassigned_finished"], float)
        assert scan["n_finished_windowed"].shape == scan["unassigned_finished"].shape == (3,)
    columns = 1 + 2 * (2 * 2 + 1) + 3 + sqc  # head, the fractions and their standard errors, hops, frustrated, drift; sqc: the unassigned fraction
    assert all(len(line.split()) == columns for line in scan["lines"]) and len(run["scattering_line"].split()) == 1 + 2 * 2 + 1 + sqc


def test_every_method_makes_the_calls_it_made(ran):
    """the literal sequences: those of test_hop_mash_host.test_the_other_methods_make_the_calls_they_made, and for "sqc" what the loops of
    their own recorded before they were merged into these"""
    step = ran["fssh"][0][1]["output_step"]
    assert step == 5 and all(ran[name][0][1]["output_step"] == step for name in NAMES)
    calls = {name: tuple(api.calls for api, _ in ran[name]) for name in NAMES}
    assert calls["fssh"] == (
        [("sample", 48), ("observe",), ("evolve", 0, 5), ("observe",), ("evolve", 5, 5), ("observe",)],
        [("sample_groups", 3, 4), ("observe_groups",), ("evolve_groups", 0, 128), ("observe_groups",), ("evolve_groups", 128, 128), ("observe_groups",)])
    assert calls["ehrenfest"] == (
        [("sample", 48), ("observe_mf",), ("evolve_mf", 5), ("observe_mf",), ("evolve_mf", 5), ("observe_mf",)],
        [("sample_groups", 3, 4), ("observe_groups_mf",), ("evolve_groups_mf", 128), ("observe_groups_mf",), ("evolve_groups_mf", 128), ("observe_groups_mf",)])
    assert calls["sqc"] == (
        [("sample_sqc", 48, 1, THIRD), ("observe_sqc", 1, THIRD), ("evolve_sqc", 5, THIRD), ("observe_sqc", 1, THIRD), ("evolve_sqc", 5, THIRD),
         ("observe_sqc", 1, THIRD)],
        [("sample_groups_sqc", 3, 4, 1, THIRD), ("observe_groups_sqc", 1, THIRD), ("evolve_groups_sqc", 128, THIRD), ("observe_groups_sqc", 1, THIRD),
         ("evolve_groups_sqc", 128, THIRD), ("observe_groups_sqc", 1, THIRD)])
    assert calls["mash"] == (
        [("sample_mash", 48), ("observe",), ("evolve_mash", 5), ("observe",), ("evolve_mash", 5), ("observe",)],
        [("sample_groups_mash", 3, 4), ("observe_groups",), ("evolve_groups_mash", 128), ("observe_groups",), ("evolve_groups_mash", 128), ("observe_groups",)])
    api = HN.NumpyHopApi()  # knows neither hop_sample_mash nor hop_evolve_mf: an attribute is looked up when its method calls it
    hopping.run(api, max_outputs=3, **RUN)
    assert api.calls == calls["fssh"][0]


def test_only_the_table_and_its_check_know_a_method_by_name():
    assert tuple(hopping.TABLE) == NAMES == hopping.METHODS + (hopping.SQC, hopping.MASH)
    assert all(isinstance(m, hopping.Method) for m in hopping.TABLE.values())
    for m in hopping.TABLE.values():  # names of api attributes and functions of the api's results, never a bound method of an api
        assert all(isinstance(getattr(m, field), str) for field in ("sample", "evolve", "observe"))
    source = inspect.getsource(hopping)
    for gone in ("mean_field", "_run_sqc", "_scan_sqc", "== MASH", "== SQC", "!= SQC", "!= MASH"):
        assert gone not in source, gone
    functions = {node.name: node for node in ast.parse(source).body if isinstance(node, ast.FunctionDef)}
    assert {"run", "scan", "_method"} <= set(functions)
    for name, function in functions.items():
        body = function.body[1:] if ast.get_docstring(function) is not None else function.body
        nodes = [n for statement in body for n in ast.walk(statement)]
        if name != "_method":  # every decision goes through the record
            assert not [n.id for n in nodes if isinstance(n, ast.Name) and n.id in ("SQC", "MASH", "METHODS", "TABLE")], name
            assert not [n.value for n in nodes if isinstance(n, ast.Constant) and n.value in NAMES], name
        if name in ("run", "scan"):  # one loop each, and nothing delegated to a second copy of it
            assert sum(isinstance(n, ast.While) for n in nodes) == 1, name
            called = {n.func.id for n in nodes if isinstance(n, ast.Call) and isinstance(n.func, ast.Name)}
            assert not [f for f in called & set(functions) if any(isinstance(n, ast.While) for n in ast.walk(functions[f]))], name
