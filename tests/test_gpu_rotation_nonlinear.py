"""tmi_ba_estimate_global_rotations_nonlinear on the device against the numpy model
(tests/rotation_nonlinear_model.py) on the inputs of tests/rotation_nonlinear_cases.py.

Held cases (fixed_view >= 0): tests/test_rotation_nonlinear_cpu.py holds the model, on these same inputs, to a smallest
decision margin above 1e-6, so the trajectory -- every step's outcome, the iteration count, the termination, the number
of factorisations -- is compared with equality, and costs, radii, rotations and residuals at the relative tolerance of
the project's device-versus-model comparisons, 1e-9: the factorisation's summation order is not numpy's.

Free cases (fixed_view = -1, the reference's problem): the normal matrix has a three-dimensional null space that only the
LM diagonal lifts, and rounding in the gradient's gauge component is amplified by up to radius / A_ii, so the rotations
themselves are not comparable.  Every real-valued gauge-invariant output is -- the loop rotations R2 R1^T as matrices, the
residuals, the cost and radius traces, and the rotations after alignment by the one rotation that best maps the device's
onto the model's -- within max(1e-9, 100 x MODEL_SPREAD), MODEL_SPREAD being the same measure between the model's two
linear-solve paths and 100 the margin for a different but fixed summation order that
tests/test_gpu_two_view_calibrated.py uses.  The decisions are compared with equality wherever the model's margin is above
1e-6, which the CPU test shows to be every free case (cases.FREE_DECISIONS_NOT_COMPARED is empty).

Shapes: orders 6, 9, 66 and 129 (one past a 64-column panel, one past two), a shuffled path of 70, a star whose hub row
(300 edges) is longer than a workgroup, order 900 with a fifth of the edges gross outliers (the negative-trace branches),
a root starting at exactly zero, unmarked views, an exactly zero error rotation (k = 2), 0 and 1 iterations."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402
import rotation_nonlinear_cases as cases  # noqa: E402
import rotation_nonlinear_model as model  # noqa: E402
from theiasfm_amd import abi, lib  # noqa: E402

pytestmark = pytest.mark.gpu
RTOL = 1e-9
SPREAD_MARGIN = 100.0
UNSUPPORTED = 5


@pytest.fixture(scope="module")
def L():
    entry.build_engine()
    return lib.load()


def _batch(case):
    return abi.ViewPairBatch(None, case["view1"], case["view2"], case["rel"], None, case["gt"].shape[0])


def _device(case, **kw):
    return lib.estimate_global_rotations_nonlinear(_batch(case), case["start"],
                                                   abi.nonlinear_rotation_options(**case["options"]), case["view_given"], **kw)


def _same_decisions(name, dev, base):
    s = dev["summary"]
    assert dev["outcomes"].tolist() == base["outcomes"].tolist()
    assert (s.num_iterations, s.termination, s.num_factorizations) == \
        (base["iterations"], base["termination"], base["factorizations"])
    assert bool(s.usable)
    assert s.num_successful_steps == int((base["outcomes"][1:] == 1).sum())
    assert s.num_unsuccessful_steps == int((base["outcomes"][1:] <= 0).sum())


def _common(case, dev, base):
    s = dev["summary"]
    assert (s.num_views, s.num_pairs) == (base["num_views"], base["num_pairs"])
    assert (s.initial_cost, s.final_cost) == (dev["costs"][0], dev["costs"][-1])
    outside = np.setdiff1d(np.arange(case["gt"].shape[0]), cases.used_views(case))
    assert dev["rotations"][outside].tobytes() == case["start"][outside].tobytes()  # never written
    if s.num_iterations:
        assert s.kernel_seconds > 0 and s.seconds >= s.kernel_seconds
        assert s.kernel_seconds == pytest.approx(s.factor_seconds + s.substitution_seconds + s.graph_seconds)


@pytest.mark.parametrize("name", cases.HELD)
def test_held_case_equals_the_model(L, name):
    case, base = cases.expected(name)
    dev = _device(case)
    s = dev["summary"]
    diff = float(np.abs(dev["rotations"] - base["rotations"]).max())
    cost_diff = float((np.abs(dev["costs"] - base["costs"]) / np.maximum(np.abs(base["costs"]), 1e-300)).max())
    print("%s: %d iterations (model %d), termination %d (model %d), outcomes %s, rotations differ by %.3e, costs by "
          "%.3e relative, residuals by %.3e" % (name, s.num_iterations, base["iterations"], s.termination,
                                                base["termination"], dev["outcomes"].tolist(), diff, cost_diff,
                                                float(np.abs(dev["residuals"] - base["residuals"]).max())))
    _same_decisions(name, dev, base)
    _common(case, dev, base)
    np.testing.assert_allclose(dev["costs"], base["costs"], rtol=RTOL, atol=0.0)
    np.testing.assert_allclose(dev["radii"], base["radii"], rtol=RTOL, atol=0.0)
    # relative to the size of the vectors: |angle-axis| and |residual| are of order 1 and at most pi
    np.testing.assert_allclose(dev["rotations"], base["rotations"], rtol=0.0,
                               atol=RTOL * max(float(np.abs(base["rotations"]).max()), 1e-300))
    np.testing.assert_allclose(dev["residuals"], base["residuals"], rtol=0.0,
                               atol=RTOL * max(float(np.abs(base["residuals"]).max()), 1e-300))
    held = case["options"]["fixed_view"]
    assert dev["rotations"][held].tobytes() == case["start"][held].tobytes()


@pytest.mark.parametrize("name", cases.FREE)
def test_free_case_equals_the_model_in_what_the_gauge_leaves(L, name):
    case, base = cases.expected(name)
    dev = _device(case)
    s = dev["summary"]
    spread = cases.model_spread(name)
    allowed = max(RTOL, SPREAD_MARGIN * spread)
    used = cases.used_views(case)
    diff = model.gauge_invariant_difference(dev, base, case["view1"], case["view2"], used)
    raw = float(np.abs(dev["rotations"] - base["rotations"]).max())
    print("%s: %d iterations (model %d), termination %d (model %d), outcomes %s, gauge-invariant difference %.3e, "
          "MODEL_SPREAD %.3e, ratio to the allowed %.3e: %.3e; raw rotations differ by %.3e" %
          (name, s.num_iterations, base["iterations"], s.termination, base["termination"], dev["outcomes"].tolist(), diff,
           spread, allowed, diff / allowed, raw))
    if name not in cases.FREE_DECISIONS_NOT_COMPARED:
        assert base["min_margin"] > 1e-6
        _same_decisions(name, dev, base)
        assert dev["costs"].size == base["costs"].size
    _common(case, dev, base)
    assert diff <= allowed


def test_two_calls_give_the_same_bytes(L):
    for name in ("random 300/1500, a fifth outliers, free", "star of 300, held", "shuffled path of 70, free"):
        case = cases.expected(name)[0]
        a, b = _device(case), _device(case)
        for key in ("rotations", "residuals", "costs", "radii", "outcomes"):
            assert a[key].tobytes() == b[key].tobytes(), (name, key)


def test_a_start_is_not_overwritten_at_the_cap_and_is_on_success(L, monkeypatch):
    case = cases.expected("zero-start root, free")[0]
    batch = _batch(case)  # (owns the arrays cb points into)
    cb = batch.as_c()
    opt = abi.nonlinear_rotation_options(**case["options"])
    s = abi.CNonlinearRotationSummary()
    rot = case["start"].copy()
    monkeypatch.setenv("TMI_BA_ROTATION_MAX_ORDER", "3")
    rc = L.tmi_ba_estimate_global_rotations_nonlinear(C.byref(cb), C.byref(opt), None, -1, rot.ctypes.data, None, None, None,
                                                      None, C.byref(s))
    assert rc == UNSUPPORTED and rot.tobytes() == case["start"].tobytes()
    monkeypatch.delenv("TMI_BA_ROTATION_MAX_ORDER")
    rc = L.tmi_ba_estimate_global_rotations_nonlinear(C.byref(cb), C.byref(opt), None, -1, rot.ctypes.data, None, None, None,
                                                      None, C.byref(s))  # every optional output NULL
    assert rc == 0 and s.usable and rot.tobytes() != case["start"].tobytes()
    assert rot.tobytes() == _device(case)["rotations"].tobytes()
    assert rot.tobytes() == _device(case, want_outputs=False)["rotations"].tobytes()


def test_the_two_refusals(L):
    case = cases.expected("triangle, free")[0]
    good = _batch(case)
    V = good.num_views
    empty = abi.ViewPairBatch(None, case["view1"][:0], case["view2"][:0], case["rel"][:0], None, V)
    with pytest.raises(lib.EngineError) as e:
        lib.estimate_global_rotations_nonlinear(empty, case["start"])
    assert e.value.status == 1
    with pytest.raises(lib.EngineError) as e:
        lib.estimate_global_rotations_nonlinear(good, case["start"], view_given=np.zeros(V, dtype=np.uint8))
    assert e.value.status == 1
    # marked views without an edge between two of them: the reference solves an empty problem; nothing is written
    given = np.array([1, 0, 0], dtype=np.uint8)
    out = lib.estimate_global_rotations_nonlinear(good, case["start"], view_given=given)
    assert out["rotations"].tobytes() == case["start"].tobytes()
    assert (out["summary"].num_pairs, out["summary"].termination, out["summary"].usable) == (0, 0, 1)


def test_pipeline_spanning_tree_then_nonlinear(L):
    """OrientationsFromMaximumSpanningTree, then this call, on a noisy graph: the summed SoftLOne cost drops and the
    largest loop-rotation error against the ground truth does not grow."""
    rng = np.random.default_rng(101)
    V, E = 40, 160
    gt, v1, v2, rel = model.scene_on_pairs(V, model.random_pairs(V, E, rng), 0.03, 102)
    batch = abi.ViewPairBatch(None, v1, v2, rel, None, V)
    tree = lib.orientations_from_maximum_spanning_tree(batch, rng.integers(30, 200, size=E).astype(np.int32))
    start = tree["orientation"]
    assert (start == 0.0).all(axis=1).sum() == 1  # the root
    out = lib.estimate_global_rotations_nonlinear(batch, start)
    s = out["summary"]

    def loop_error(rot):
        return float(np.abs(model.loop_rotations(rot, v1, v2) - model.loop_rotations(gt, v1, v2)).max())

    def cost(rot):
        r = model.pairwise_rotation_error(rot[v1], rot[v2], rel)[0]
        return float((0.5 * model.soft_l_one((r * r).sum(axis=1), 0.1)[0]).sum())

    print("pipeline: cost %.6e -> %.6e in %d iterations (termination %d); largest loop-rotation error %.3e -> %.3e" %
          (s.initial_cost, s.final_cost, s.num_iterations, s.termination, loop_error(start), loop_error(out["rotations"])))
    assert s.termination == 0 and s.final_cost < s.initial_cost
    assert cost(start) == pytest.approx(s.initial_cost, rel=1e-9) and cost(out["rotations"]) == pytest.approx(s.final_cost, rel=1e-9)
    assert loop_error(out["rotations"]) <= loop_error(start)
