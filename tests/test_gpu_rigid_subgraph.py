"""tmi_ba_extract_parallel_rigid_subgraph on the device against the numpy model (tests/rigid_subgraph_model.py) on the
scenes of tests/rigid_subgraph_cases.py, none excluded: the decisions (keep, component_size, null_dimension,
fixed_view) exactly, the null space as a projector within max(1e-12, 100 x MODEL_SPREAD) -- the factor 100 is for the
device's other summation order and iteration count -- with |L N| below the call's stop tolerance and N^T N = I to 1e-12;
the block widths the scenes are built to reach; the refusal that writes nothing; masked and isolated views; the same
bytes from two calls; and the C++ shim on the device.

Measured on one MI355X: see the figures there.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rigid_subgraph_cases as cases  # noqa: E402
from shim_build import compile_shim  # noqa: E402
from theiasfm_amd import abi, lib  # noqa: E402

pytestmark = pytest.mark.gpu

RUNNABLE = [c["name"] for c in cases.scenes() if "status" not in c["expect"]]


def _batch(case):
    return abi.ViewPairBatch(case["orientation"], case["view1"], case["view2"], None, case["position2"])


def _run(case, **kw):
    return lib.extract_parallel_rigid_subgraph(_batch(case), abi.rigid_subgraph_options(**case["options"]),
                                               view_mask=case["view_mask"], **kw)


def _case(name):
    return next(c for c in cases.scenes() if c["name"] == name)


_results = {}


def _result(name):
    if name not in _results:
        _results[name] = _run(_case(name), want_null_space=True)
    return _results[name]


@pytest.mark.parametrize("name", RUNNABLE)
def test_decisions_equal_the_model(name):
    got, want = _result(name), cases.modelled(name)
    s = got["summary"]
    print(name, "k", s.null_dimension, "m", s.block_width, "iterations", s.iterations, "fixed", s.fixed_view, "kept",
          s.num_kept, "residual %.3e tolerance %.3e" % (s.max_residual, s.stop_tolerance),
          "values %.3e | %.3e of %.3e" % (s.largest_null_value, s.smallest_other_value, s.largest_diagonal))
    assert s.null_dimension == want["null_dimension"]
    assert np.array_equal(got["keep"], want["keep"])
    assert np.array_equal(got["component_size"], want["component_size"])
    assert s.fixed_view == want["fixed_view"]
    assert s.num_kept == int(want["keep"].sum())
    assert s.num_views == len(want["view_of"]) and s.order == 3 * s.num_views
    expect = _case(name)["expect"]
    if "kept" in expect:
        assert np.flatnonzero(got["keep"]).tolist() == expect["kept"]
    if "null_dimension" in expect:
        assert s.null_dimension == expect["null_dimension"]
    if "block_width" in expect:
        assert s.block_width == expect["block_width"]


@pytest.mark.parametrize("name", RUNNABLE)
def test_null_space(name):
    got, want = _result(name), cases.modelled(name)
    N, s = got["null_space"], got["summary"]
    assert N.shape == want["null_space"].shape
    bound = max(1e-12, 100.0 * cases.model_spread())
    difference = float(np.abs(N @ N.T - want["null_space"] @ want["null_space"].T).max())
    residual = float(np.linalg.norm(want["laplacian"] @ N, axis=0).max()) if N.shape[1] else 0.0
    orthogonality = float(np.abs(N.T @ N - np.eye(N.shape[1])).max()) if N.shape[1] else 0.0
    print(name, "projector difference %.3e (bound %.3e)  |L N| %.3e (stop tolerance %.3e)  |N^T N - I| %.3e"
          % (difference, bound, residual, s.stop_tolerance, orthogonality))
    assert difference <= bound
    assert residual < s.stop_tolerance
    assert orthogonality <= 1e-12
    for c in range(N.shape[1]):  # the sign rule: the first entry of largest magnitude is positive
        assert N[np.argmax(np.abs(N[:, c])), c] > 0.0


def test_the_block_doubles_when_the_null_space_fills_it():
    assert _result("chain6")["summary"].block_width == 16 and _result("chain6")["summary"].null_dimension == 8


def test_too_large_a_null_space_is_refused_and_nothing_is_written():
    case = _case("chain12_refused")
    V = case["orientation"].shape[0]
    outputs = dict(keep=np.full(V, 7, dtype=np.uint8), component_size=np.full(V, -5, dtype=np.int32),
                   null_space=np.full(3 * V * 8, 0.25))
    with pytest.raises(lib.EngineError) as e:
        _run(case, want_null_space=True, outputs=outputs)
    assert e.value.status == abi.ERR_NULL_SPACE_TOO_LARGE
    assert np.all(outputs["keep"] == 7) and np.all(outputs["component_size"] == -5) and np.all(outputs["null_space"] == 0.25)
    # the same chain with room for it
    free = dict(case, options={})
    got = _run(free)
    assert got["summary"].null_dimension == 14 and got["summary"].block_width == 16
    assert np.array_equal(got["keep"], cases.modelled("chain12_refused")["keep"])


def test_masked_and_isolated_views_come_back_zero():
    got = _result("isolated_and_masked")
    assert got["keep"][2] == 0 and got["keep"][4] == 0 and got["component_size"][2] == 0 and got["component_size"][4] == 0
    assert got["summary"].num_views == 8


def test_iteration_cap_is_a_status():
    with pytest.raises(lib.EngineError) as e:
        _run(dict(_case("chain6"), options=dict(max_iterations=1)))
    assert e.value.status == abi.ERR_NOT_CONVERGED


@pytest.mark.parametrize("name", ["many_bad_rotations", "core_with_leaves"])
def test_two_calls_give_the_same_bytes(name):
    a, b = _result(name), _run(_case(name), want_null_space=True)
    for key in ("keep", "component_size", "null_space"):
        assert a[key].tobytes() == b[key].tobytes(), key


def test_rigid_subgraph_shim_on_the_device(tmp_path):
    exe = compile_shim(tmp_path, "test_rigid_subgraph_shim.cc", ["rigid_subgraph_ops.cc"])
    p = subprocess.run([exe, "--need-device"], capture_output=True, text=True, timeout=600)
    print(p.stdout, p.stderr)
    assert p.returncode == 0 and "rigid subgraph shim: OK" in p.stdout, p.stdout + p.stderr
