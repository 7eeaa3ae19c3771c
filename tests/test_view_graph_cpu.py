"""The view-graph calls without a GPU: the CPU model (tests/view_graph_model.py) on the reference's own test cases and
on graphs whose answer is known by hand, the argument checks of tmi_ba_largest_connected_component and
tmi_ba_orientations_from_maximum_spanning_tree (status 1 before the device is looked for, with every output untouched;
status 2 for a valid batch where there is no device), and the Python side of the ABI."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402
import view_graph_cases as cases  # noqa: E402
import view_graph_model as model  # noqa: E402
from theiasfm_amd import abi, lib  # noqa: E402

INVALID_ARGUMENT, NO_DEVICE = 1, 2


@pytest.fixture(scope="module")
def L():
    entry.build_engine()
    return lib.load()


# ---- the reference's cases on the model ----------------------------------------------------------------------------
@pytest.mark.parametrize("name,edges_left,removed", [
    ("reference_one_component", 3, set()),
    ("reference_two_components", 3, {5, 6, 7}),
    ("reference_three_components", 3, {5, 6, 7, 8}),
])
def test_remove_disconnected_view_pairs(name, edges_left, removed):
    """remove_disconnected_view_pairs_test.cc:49-96."""
    c = cases.component_cases()[name]
    r = cases.component_model(name)
    assert r.num_pairs_kept == edges_left and r.largest_label == 0 and r.largest_num_views == 4
    assert r.keep.tolist() == [1, 1, 1] + [0] * (len(c.v1) - 3)
    with_edge = set(c.v1.tolist()) | set(c.v2.tolist())
    assert {v for v in with_edge if not r.in_largest[v]} == removed and r.num_views_removed == len(removed)
    assert r.label.tolist()[:4] == [0, 0, 0, 0] and r.label[4] == 4  # view 4 has no edge: its own component


@pytest.mark.parametrize("name", ["reference_4_6", "reference_50_100"])
def test_orientations_from_view_graph(name):
    """orientations_from_maximum_spanning_tree_test.cc:156-165: noise-free, every edge's relative rotation recovered
    within the reference's 1e-12."""
    c = cases.tree_cases()[name]
    r = cases.tree_model(name)
    assert r.usable and r.num_tree_pairs == c.V - 1 and (r.depth >= 0).all()
    worst = 0.0
    for a, b in zip(c.v1, c.v2):
        d = model.relative_rotation(c.gt[a], c.gt[b]) - model.relative_rotation(r.orientation[a], r.orientation[b])
        worst = max(worst, float(np.linalg.norm(d)))
    print(name, "worst relative-rotation error", worst)
    assert worst < 1e-12


# ---- by hand -----------------------------------------------------------------------------------------------------------
def test_k8_with_equal_weights_is_the_star_at_view_0():
    """Every weight ties, so the order is (view1, view2) ascending: (0, 1) .. (0, 7) come first and span the graph."""
    c = cases.tree_cases()["k8_equal_weights"]
    r = cases.tree_model("k8_equal_weights")
    assert [(int(a), int(b)) for a, b, t in zip(c.v1, c.v2, r.in_tree) if t] == [(0, k) for k in range(1, 8)]
    assert r.parent.tolist() == [-1] + [0] * 7 and r.depth.tolist() == [0] + [1] * 7 and r.root_view == 0
    assert r.parent_pair.tolist() == [-1, 0, 1, 2, 3, 4, 5, 6] and r.tree_depth == 1
    for k in range(1, 8):  # one step from the identity: the edge's own rotation
        assert model.rotation_difference(r.orientation[k], c.rotation2[k - 1]) < 1e-14


def test_cycle_leaves_its_lightest_edge_out():
    c = cases.tree_cases()["cycle_lightest_left_out"]
    r = cases.tree_model("cycle_lightest_left_out")
    assert r.in_tree.tolist() == [1, 1, 0, 1, 1, 1] and int(c.weight[2]) == int(c.weight.min())
    # 0 is the root; the cycle is cut between 2 and 3
    assert r.parent.tolist() == [-1, 0, 1, 4, 5, 0] and r.depth.tolist() == [0, 1, 2, 3, 2, 1]


def test_component_rules():
    r = cases.component_model("equal_sizes_tie")
    assert r.label.tolist() == [0, 1, 1, 1, 4, 4, 4] and r.largest_label == 1 and r.keep.tolist() == [0, 0, 1, 1]
    assert (r.num_components, r.num_views_removed, r.num_pairs_removed) == (2, 3, 2)
    r = cases.component_model("no_alive_edge")
    assert r.largest_label == -1 and not r.keep.any() and not r.in_largest.any() and r.label.tolist() == [0, 1, 2, 3]
    assert (r.num_components, r.largest_num_views, r.num_views_removed) == (0, 0, 0)
    r = cases.component_model("random_2000")
    assert r.num_components == 40 and (np.bincount(r.label) == 1).sum() == 100  # the isolated views
    c = cases.root_outside_case()
    with pytest.raises(ValueError):
        model.spanning_tree(c.V, c.v1, c.v2, c.weight, c.rotation2, c.mask, c.root)


def test_rotation_formulas_at_their_branches():
    rng = np.random.default_rng(0)
    for scale in (0.0, 1e-9, 1e-4, 1.0, np.pi - 1e-6, np.pi - 1e-9):
        for _ in range(20):
            a = rng.normal(size=3)
            a *= scale / np.linalg.norm(a)
            R = model.angle_axis_to_rotation_matrix(a)
            assert np.abs(R @ R.T - np.eye(3)).max() < 1e-14 + 4 * scale * scale * (scale < 1e-3)  # (first order below sqrt(eps))
            assert model.rotation_difference(model.rotation_matrix_to_angle_axis(R), a) < 1e-14


# ---- the ABI ---------------------------------------------------------------------------------------------------------
def test_symbols_are_exported(L):
    for name in ("tmi_ba_largest_connected_component", "tmi_ba_orientations_from_maximum_spanning_tree"):
        assert name in lib.EXPORTS and hasattr(L, name)


SENTINEL = 77


class Outputs:
    """Every output of both calls, preset to a sentinel."""

    def __init__(self, V, E):
        self.label = np.full(V, SENTINEL, np.int32)
        self.in_largest = np.full(V, SENTINEL, np.uint8)
        self.keep = np.full(E, SENTINEL, np.uint8)
        self.orientation = np.full((V, 3), float(SENTINEL))
        self.parent = np.full(V, SENTINEL, np.int32)
        self.parent_pair = np.full(V, SENTINEL, np.int32)
        self.depth = np.full(V, SENTINEL, np.int32)
        self.in_tree = np.full(E, SENTINEL, np.uint8)
        self.cs = abi.CViewGraphComponentSummary()
        self.ts = abi.CSpanningTreeSummary()
        C.memset(C.byref(self.cs), SENTINEL, C.sizeof(self.cs))
        C.memset(C.byref(self.ts), SENTINEL, C.sizeof(self.ts))

    def untouched(self):
        arrays = (self.label, self.in_largest, self.keep, self.orientation, self.parent, self.parent_pair, self.depth,
                  self.in_tree)
        return all((a == SENTINEL).all() for a in arrays) and \
            all(b == SENTINEL for b in bytes(self.cs) + bytes(self.ts))


def _valid():
    return cases.tree_cases()["root_first"]


def _components(L, cb, out, mask=None, summary=True):
    return L.tmi_ba_largest_connected_component(
        None if cb is None else C.byref(cb), None if mask is None else mask.ctypes.data, -1, out.label.ctypes.data,
        out.in_largest.ctypes.data, out.keep.ctypes.data, C.byref(out.cs) if summary else None)


def _tree(L, cb, out, weight, mask=None, root=-1, summary=True):
    return L.tmi_ba_orientations_from_maximum_spanning_tree(
        None if cb is None else C.byref(cb), None if weight is None else weight.ctypes.data,
        None if mask is None else mask.ctypes.data, root, -1, out.orientation.ctypes.data, out.parent.ctypes.data,
        out.parent_pair.ctypes.data, out.depth.ctypes.data, out.in_tree.ctypes.data,
        C.byref(out.ts) if summary else None)


def _null(cb, name):
    setattr(cb, name, C.cast(None, type(getattr(cb, name))))


def _set(name, index, value):
    def edit(B, cb):
        getattr(B, name).reshape(-1)[index] = value
    return edit


# edits of a valid batch that both calls must refuse
BAD_BATCHES = {
    "negative num_views": lambda B, cb: setattr(cb, "num_views", -1),
    "negative num_pairs": lambda B, cb: setattr(cb, "num_pairs", -3),
    "no pair_view1": lambda B, cb: _null(cb, "pair_view1"),
    "no pair_view2": lambda B, cb: _null(cb, "pair_view2"),
    "view index too large": _set("pair_view2", 1, 12),
    "view index negative": _set("pair_view1", 0, -1),
    "view paired with itself": _set("pair_view2", 2, 4),  # edge 2 is (4, 6)
}


def test_argument_errors_come_before_the_device_and_touch_nothing(L):
    """Each of these is TMI_BA_ERR_INVALID_ARGUMENT (1), never TMI_BA_ERR_NO_DEVICE (2), with a message and with every
    output, the summary included, as it was."""
    c = _valid()

    def check(name, call, edit=None, **kw):
        B = cases.batch(c)
        cb = B.as_c()
        if edit:
            edit(B, cb)
        out = Outputs(c.V, len(c.v1))
        assert call(L, cb, out, **kw) == INVALID_ARGUMENT, name
        assert L.tmi_ba_last_error(), name
        assert out.untouched(), name

    w = c.weight.copy()
    for name, edit in BAD_BATCHES.items():
        check(name, _components, edit)
        check(name, _tree, edit, weight=w)
    check("no weights", _tree, weight=None)
    check("no pair_rotation2", _tree, lambda B, cb: _null(cb, "pair_rotation2"), weight=w)
    negative = w.copy()
    negative[3] = -1
    check("negative weight on an alive edge", _tree, weight=negative)
    alive = np.ones(len(w), np.uint8)
    check("negative weight on an alive edge under a mask", _tree, weight=negative, mask=alive)
    for root in (-2, c.V, c.V + 5):
        check("root_view out of range", _tree, weight=w, root=root)
    for call, kw in ((_components, {}), (_tree, dict(weight=w))):
        out = Outputs(c.V, len(c.v1))
        assert call(L, None, out, **kw) == INVALID_ARGUMENT and out.untouched()
        assert call(L, cases.batch(c).as_c(), out, summary=False, **kw) == INVALID_ARGUMENT and out.untouched()


def test_a_valid_batch_reaches_the_device(L):
    """Without a device a valid batch is TMI_BA_ERR_NO_DEVICE (2) and nothing is written; with one it is OK."""
    have = L.tmi_ba_device_count() > 0
    want = 0 if have else NO_DEVICE
    c = _valid()
    dead = np.ones(len(c.weight), np.uint8)
    dead[3] = 0
    negative = c.weight.copy()
    negative[3] = -1  # a negative weight on a masked edge is not an error
    for case, kw in ((c, {}), (c, dict(weight=negative, mask=dead)), (cases.component_cases()["one_view_no_edge"], {}),
                     (cases.root_outside_case(), {})):
        B = cases.batch(case)
        out = Outputs(case.V, len(case.v1))
        assert _components(L, B.as_c(), out, mask=kw.get("mask")) == want
        assert have or out.untouched()
        out = Outputs(case.V, len(case.v1))
        st = _tree(L, B.as_c(), out, kw.get("weight", case.weight), mask=kw.get("mask"), root=case.root)
        # (a root outside the largest component is found on the device)
        assert st == (INVALID_ARGUMENT if have and case.root == 5 else want)
        assert (have and st == 0) or out.untouched()
    if not have:
        with pytest.raises(lib.EngineError) as e:
            lib.largest_connected_component(cases.batch(c))
        assert e.value.status == NO_DEVICE
        with pytest.raises(lib.EngineError) as e:
            lib.orientations_from_maximum_spanning_tree(cases.batch(c), c.weight)
        assert e.value.status == NO_DEVICE
    with pytest.raises(ValueError):
        lib.largest_connected_component(cases.batch(c), pair_mask=np.ones(3))
    with pytest.raises(ValueError):
        lib.orientations_from_maximum_spanning_tree(cases.batch(c), c.weight[:-1])


def test_struct_layout_matches_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "theia_mi355_ba.h"\n'
        'int main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(tmi_ba_view_graph_component_summary),'
        "offsetof(tmi_ba_view_graph_component_summary, num_views_removed),"
        "offsetof(tmi_ba_view_graph_component_summary, seconds),"
        "offsetof(tmi_ba_view_graph_component_summary, kernel_seconds), sizeof(tmi_ba_spanning_tree_summary),"
        "offsetof(tmi_ba_spanning_tree_summary, num_tree_pairs), offsetof(tmi_ba_spanning_tree_summary, root_view),"
        "offsetof(tmi_ba_spanning_tree_summary, usable));return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    S, T = abi.CViewGraphComponentSummary, abi.CSpanningTreeSummary
    assert got == [C.sizeof(S), S.num_views_removed.offset, S.seconds.offset, S.kernel_seconds.offset, C.sizeof(T),
                   T.num_tree_pairs.offset, T.root_view.offset, T.usable.offset]
