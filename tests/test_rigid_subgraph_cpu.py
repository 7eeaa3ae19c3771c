"""ExtractMaximallyParallelRigidSubgraph without a device: the numpy model (tests/rigid_subgraph_model.py) on the scenes
of tests/rigid_subgraph_cases.py, the condition on those scenes that makes the device comparison exact, the C ABI's
argument checks and defaults, and the host side of the C++ shim on a stubbed call.

The two null-space paths of the model (eigh of L, the right singular vectors of the explicit A) must give the same
keep, component_size and k on every scene.  MODEL_SPREAD, the largest entry of the difference of their projectors
N N^T over the scenes, is 2.2e-15 (printed by test_model_paths_agree); tests/test_gpu_rigid_subgraph.py bounds the
device's projector by max(1e-12, 100 x MODEL_SPREAD).

The condition on the inputs: every decision of every scene has a margin -- null eigenvalues below null_tolerance / 1e3
and the others above 1e3 x null_tolerance (relative to the largest diagonal entry of L), row norms < 1e-12 or > 1e-8,
cosine distances < 1e-7 or > 1e-3.  A scene that fails it is to be replaced, not excused: the GPU test excludes none.
"""
import ctypes as C
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

NAMES = [c["name"] for c in cases.scenes()]
NULL_TOLERANCE = 1e-9
INVALID, NO_DEVICE, UNSUPPORTED = 1, 2, 5


def _case(name):
    return next(c for c in cases.scenes() if c["name"] == name)


@pytest.mark.parametrize("name", NAMES)
def test_model_paths_agree(name):
    a, b = cases.modelled(name, "eigh"), cases.modelled(name, "svd")
    assert a["null_dimension"] == b["null_dimension"]
    assert np.array_equal(a["keep"], b["keep"]) and np.array_equal(a["component_size"], b["component_size"])
    assert a["fixed_view"] == b["fixed_view"]
    spread = float(np.abs(a["null_space"] @ a["null_space"].T - b["null_space"] @ b["null_space"].T).max())
    print(name, "k", a["null_dimension"], "spread %.3e" % spread, "MODEL_SPREAD %.3e" % cases.model_spread())
    assert spread <= cases.model_spread() <= 1e-13  # (the paths differ by rounding only)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("path", ["eigh", "svd"])
def test_every_decision_has_a_margin(name, path):
    m = cases.modelled(name, path)["margins"]
    print(name, path, {k: "%.3e" % v for k, v in m.items()})
    assert m["null_max"] < NULL_TOLERANCE / 1e3 and m["other_min"] > 1e3 * NULL_TOLERANCE
    assert m["norm_below_max"] < 1e-12 and m["norm_above_min"] > 1e-8
    assert m["cos_below_max"] < 1e-7 and m["cos_above_min"] > 1e-3


@pytest.mark.parametrize("name", NAMES)
def test_scenes_show_what_they_are_built_for(name):
    case, got = _case(name), cases.modelled(name)
    expect = case["expect"]
    if "null_dimension" in expect:
        assert got["null_dimension"] == expect["null_dimension"]
    if "kept" in expect:
        assert np.flatnonzero(got["keep"]).tolist() == expect["kept"]
    if "min_pairs_left" in expect:  # extract_maximally_parallel_rigid_subgraph_test.cc:169-170
        left = int(np.sum(got["keep"][case["view1"]] & got["keep"][case["view2"]]))
        assert left >= expect["min_pairs_left"] and int(got["keep"].sum()) == case["orientation"].shape[0]
    if case["view_mask"] is not None:
        outside = np.flatnonzero(case["view_mask"] == 0)
        assert not got["keep"][outside].any() and not got["component_size"][outside].any()


def test_tie_breaks_to_the_smallest_view():
    got = cases.modelled("chain6")
    assert set(got["component_size"].tolist()) == {1} and got["fixed_view"] == 0


# ---- the C ABI without a device ----------------------------------------------------------------------------------------
def test_options_defaults_and_struct_sizes(tmp_path):
    L = lib.load()
    o = abi.CRigidSubgraphOptions()
    L.tmi_ba_rigid_subgraph_options_init(C.byref(o))
    d = abi.rigid_subgraph_options()
    for name, _ in abi.CRigidSubgraphOptions._fields_:
        assert getattr(o, name) == getattr(d, name), name
    assert (o.relative_shift, o.null_tolerance, o.max_null_dimension, o.max_iterations, o.device) == (1e-9, 1e-9, 128, 100, -1)
    with pytest.raises(AttributeError):
        abi.rigid_subgraph_options(no_such_field=1)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "theia_mi355_ba.h"\nint main(void) {\n'
                   'printf("%zu %zu\\n", sizeof(tmi_ba_rigid_subgraph_options), sizeof(tmi_ba_rigid_subgraph_summary));\n'
                   "return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    sizes = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in sizes] == [C.sizeof(abi.CRigidSubgraphOptions), C.sizeof(abi.CRigidSubgraphSummary)]
    assert abi.STATUS_NAMES[abi.ERR_NULL_SPACE_TOO_LARGE] == "NULL_SPACE_TOO_LARGE"
    assert abi.STATUS_NAMES[abi.ERR_NOT_CONVERGED] == "NOT_CONVERGED"


def _call(L, batch, options=None, keep=True, summary=True, mask=None):
    """(status, outputs untouched)."""
    V = batch.num_views if batch is not None else 1
    o = options if options is not None else abi.rigid_subgraph_options()
    k = np.full(V, 7, dtype=np.uint8)
    size = np.full(V, -5, dtype=np.int32)
    s = abi.CRigidSubgraphSummary()
    cb = batch.as_c() if batch is not None else None
    st = L.tmi_ba_extract_parallel_rigid_subgraph(C.byref(cb) if cb is not None else None,
                                                  mask.ctypes.data if mask is not None else None,
                                                  C.byref(o) if options is not False else None,
                                                  k.ctypes.data if keep else None, size.ctypes.data, None,
                                                  C.byref(s) if summary else None)
    return st, bool(np.all(k == 7) and np.all(size == -5))


def _batch(case, **changes):
    f = dict(orientation=case["orientation"], view1=case["view1"], view2=case["view2"], position2=case["position2"])
    f.update(changes)
    return abi.ViewPairBatch(f["orientation"], f["view1"], f["view2"], None, f["position2"])


def test_argument_checks():
    L = lib.load()
    case = _case("no_bad_rotations")
    good = _batch(case)
    # null pointers first
    assert _call(L, None) == (INVALID, True)
    assert _call(L, good, options=False) == (INVALID, True)
    assert _call(L, good, keep=False) == (INVALID, True)
    assert _call(L, good, summary=False) == (INVALID, True)
    # the batch
    v1 = case["view1"].copy()
    v1[3] = 99
    assert _call(L, _batch(case, view1=v1)) == (INVALID, True)
    assert _call(L, _batch(case, view1=case["view2"])) == (INVALID, True)                     # a view paired with itself
    twice = dict(view1=np.append(case["view1"], case["view2"][0]), view2=np.append(case["view2"], case["view1"][0]),
                 position2=np.vstack([case["position2"], case["position2"][:1]]))
    assert _call(L, _batch(case, **twice)) == (INVALID, True)                                 # an unordered pair twice
    bad = case["position2"].copy()
    bad[2, 1] = np.nan
    assert _call(L, _batch(case, position2=bad)) == (INVALID, True)
    bad = case["orientation"].copy()
    bad[0, 0] = np.inf
    assert _call(L, _batch(case, orientation=bad)) == (INVALID, True)
    no_orientation = abi.ViewPairBatch(None, case["view1"], case["view2"], None, case["position2"], num_views=10)
    assert _call(L, no_orientation) == (INVALID, True)
    # the batch goes before the options: both wrong, the batch's message
    assert _call(L, _batch(case, view1=v1), options=abi.rigid_subgraph_options(max_iterations=0)) == (INVALID, True)
    assert "view index out of range" in L.tmi_ba_last_error().decode()
    # the options, in the header's order
    for overrides, word in ((dict(relative_shift=-1.0), "relative_shift"), (dict(relative_shift=np.nan), "relative_shift"),
                            (dict(null_tolerance=0.0), "null_tolerance"), (dict(null_tolerance=np.inf), "null_tolerance"),
                            (dict(max_null_dimension=0), "max_null_dimension"),
                            (dict(max_null_dimension=129), "max_null_dimension"), (dict(max_iterations=0), "max_iterations"),
                            (dict(relative_shift=-1.0, max_iterations=0), "relative_shift")):
        assert _call(L, good, options=abi.rigid_subgraph_options(**overrides)) == (INVALID, True), overrides
        assert word in L.tmi_ba_last_error().decode(), overrides


def test_the_order_cap_comes_before_the_device(monkeypatch):
    L = lib.load()
    good = _batch(_case("no_bad_rotations"))
    monkeypatch.setenv("TMI_BA_ROTATION_MAX_ORDER", "29")   # n = 30
    assert _call(L, good) == (UNSUPPORTED, True)
    monkeypatch.setenv("TMI_BA_ROTATION_MAX_ORDER", "30")
    st, _ = _call(L, good)
    assert st in (0, NO_DEVICE)
    # a masked view does not count
    mask = np.ones(10, dtype=np.uint8)
    mask[9] = 0
    monkeypatch.setenv("TMI_BA_ROTATION_MAX_ORDER", "27")
    st, _ = _call(L, good, mask=mask)
    assert st in (0, NO_DEVICE)


def test_python_binding_checks_its_arrays():
    case = _case("chain6")
    with pytest.raises(ValueError):
        lib.extract_parallel_rigid_subgraph(_batch(case), outputs=dict(keep=np.zeros(3, dtype=np.uint8)))
    with pytest.raises(ValueError):
        lib.extract_parallel_rigid_subgraph(abi.ViewPairBatch(None, case["view1"], case["view2"], None, case["position2"]))


# ---- the shim's host side ---------------------------------------------------------------------------------------------
def test_rigid_subgraph_shim_host_side(tmp_path):
    """The flattening order, a graph untouched on a missing orientation or a failed call, removal of exactly the views
    that are not kept -- on a stubbed call (-DRSG_STUB_ABI), so on any machine."""
    exe = compile_shim(tmp_path, "test_rigid_subgraph_shim.cc", ["rigid_subgraph_ops.cc"], extra_flags=("-DRSG_STUB_ABI",))
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(p.stdout, p.stderr)
    assert p.returncode == 0 and "rigid subgraph shim (stubbed call): OK" in p.stdout, p.stdout + p.stderr


def test_rigid_subgraph_shim(tmp_path):
    """Whatever the machine has: without a device false and an unchanged graph, with one the full comparison."""
    exe = compile_shim(tmp_path, "test_rigid_subgraph_shim.cc", ["rigid_subgraph_ops.cc"])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(p.stdout, p.stderr)
    assert p.returncode == 0 and "OK" in p.stdout, p.stdout + p.stderr
