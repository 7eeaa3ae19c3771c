"""-m gpu: tmi_ba_largest_connected_component and tmi_ba_orientations_from_maximum_spanning_tree
(view_graph_kernels.h) against the CPU model (tests/view_graph_model.py) on the cases of tests/view_graph_cases.py.

Every integer output -- labels, masks, counts, parents, parent pairs, depths, tree flags -- must EQUAL the model's, and
two calls must give the same bytes.  Orientations are compared as rotations, by the angle of R(device) R(model)^T (the
angle-axis vector is discontinuous at pi), against

    1e-13 (view_depth + 1) rad,

which is derived, not measured: a step of the chain is two Rodrigues evaluations, a 3x3 product and one conversion
back, some tens of operations each a few units of 2.2e-16, and the device's sin, cos, atan2 and sqrt are within a
couple of ulps of numpy's.  The largest value seen on the MI355X is in DESIGN 8.15 next to the bound."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import view_graph_cases as cases  # noqa: E402
import view_graph_model as model  # noqa: E402
from theiasfm_amd import lib  # noqa: E402

pytestmark = pytest.mark.gpu

STEP_BOUND = 1e-13   # rad per step of the chain
REFERENCE_TOLERANCE = 1e-12  # orientations_from_maximum_spanning_tree_test.cc:122
SUMMARY_FIELDS = ("num_components", "largest_label", "largest_num_views", "num_pairs_kept", "num_pairs_removed",
                  "num_views_removed")


def _check_component_summary(cs, want, name):
    for f in SUMMARY_FIELDS:
        assert getattr(cs, f) == getattr(want, f), (name, f)


@pytest.mark.parametrize("name", list(cases.component_cases()))
def test_largest_component_equals_the_model(name):
    c = cases.component_cases()[name]
    want = cases.component_model(name)
    label, in_largest, keep, cs = lib.largest_connected_component(cases.batch(c), c.mask)
    assert (label == want.label).all(), name
    assert (in_largest == want.in_largest).all() and (keep == want.keep).all(), name
    _check_component_summary(cs, want, name)
    assert int(keep.sum()) == cs.num_pairs_kept and int(in_largest.sum()) == cs.largest_num_views
    again = lib.largest_connected_component(cases.batch(c), c.mask)
    for a, b in zip((label, in_largest, keep), again[:3]):
        assert a.tobytes() == b.tobytes(), name


def _run_tree(c):
    return lib.orientations_from_maximum_spanning_tree(cases.batch(c), c.weight, c.mask, c.root)


@pytest.mark.parametrize("name", list(cases.tree_cases()))
def test_spanning_tree_equals_the_model(name):
    c = cases.tree_cases()[name]
    want = cases.tree_model(name)
    got = _run_tree(c)
    ts = got["summary"]
    _check_component_summary(ts.component, want.component, name)
    assert (ts.usable, ts.num_tree_pairs, ts.tree_depth, ts.root_view) == \
        (want.usable, want.num_tree_pairs, want.tree_depth, want.root_view), name
    for key in ("in_tree", "parent", "parent_pair", "depth"):
        assert (got[key] == getattr(want, key)).all(), (name, key)
    assert ts.num_tree_pairs == ts.component.largest_num_views - 1 == int(got["in_tree"].sum())
    tree = got["in_tree"].astype(bool)
    assert int(c.weight[tree].sum()) == int(c.weight[want.in_tree.astype(bool)].sum())
    # two calls: the same bytes, the orientations included
    again = _run_tree(c)
    for key in ("in_tree", "parent", "parent_pair", "depth", "orientation"):
        assert got[key].tobytes() == again[key].tobytes(), (name, key)
    # the orientations as rotations
    in_tree_view = got["depth"] >= 0
    assert np.isnan(got["orientation"][~in_tree_view]).all()  # outside the tree: left as they were
    assert (got["orientation"][c.root if c.root >= 0 else want.root_view] == 0.0).all()
    worst = 0.0
    for v in np.flatnonzero(in_tree_view):
        d = model.rotation_difference(got["orientation"][v], want.orientation[v])
        worst = max(worst, d / (got["depth"][v] + 1))
        assert d <= STEP_BOUND * (got["depth"][v] + 1), (name, int(v), d, int(got["depth"][v]))
    print(f"{name}: views {int(in_tree_view.sum())} depth {ts.tree_depth} worst angle / (depth + 1) {worst:.3e} rad "
          f"kernel {ts.component.kernel_seconds * 1e6:.0f} us")


@pytest.mark.parametrize("name", ["reference_4_6", "reference_50_100"])
def test_reference_scenes_recover_the_relative_rotations(name):
    """VerifyOrientations of the reference's test on the device's orientations, within its own 1e-12."""
    c = cases.tree_cases()[name]
    o = _run_tree(c)["orientation"]
    worst = 0.0
    for a, b in zip(c.v1, c.v2):
        d = model.relative_rotation(c.gt[a], c.gt[b]) - model.relative_rotation(o[a], o[b])
        worst = max(worst, float(np.linalg.norm(d)))
    print(name, "worst relative-rotation error", worst)
    assert worst < REFERENCE_TOLERANCE


def test_root_outside_the_largest_component_is_an_error_with_the_outputs_untouched():
    c = cases.root_outside_case()
    B = cases.batch(c)
    cb = B.as_c()
    L = lib.load()
    import ctypes as C
    from theiasfm_amd import abi
    E = len(c.v1)
    o = np.full((c.V, 3), 77.0)
    ints = [np.full(c.V, 77, np.int32) for _ in range(3)]
    in_tree = np.full(E, 77, np.uint8)
    ts = abi.CSpanningTreeSummary()
    C.memset(C.byref(ts), 77, C.sizeof(ts))
    st = L.tmi_ba_orientations_from_maximum_spanning_tree(
        C.byref(cb), c.weight.ctypes.data, None, c.root, -1, o.ctypes.data, ints[0].ctypes.data, ints[1].ctypes.data,
        ints[2].ctypes.data, in_tree.ctypes.data, C.byref(ts))
    assert st == 1 and b"root_view" in L.tmi_ba_last_error()
    assert (o == 77.0).all() and all((a == 77).all() for a in ints) and (in_tree == 77).all()
    assert all(b == 77 for b in bytes(ts))


def test_no_alive_edge_is_not_usable_and_writes_nothing():
    c = cases.component_cases()["no_alive_edge"]
    start = np.arange(12.0).reshape(4, 3)
    got = lib.orientations_from_maximum_spanning_tree(cases.batch(c), c.weight, c.mask, view_orientation=start)
    ts = got["summary"]
    assert (ts.usable, ts.num_tree_pairs, ts.root_view, ts.component.largest_label) == (0, 0, -1, -1)
    assert (got["orientation"] == start).all() and (got["depth"] == -1).all() and not got["in_tree"].any()
    one = cases.component_cases()["one_view_no_edge"]
    ts = lib.orientations_from_maximum_spanning_tree(cases.batch(one), one.weight)["summary"]
    assert (ts.usable, ts.num_tree_pairs, ts.component.largest_label) == (0, 0, -1)
