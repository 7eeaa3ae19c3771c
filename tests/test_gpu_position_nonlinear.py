"""tmi_ba_estimate_global_positions_nonlinear on the device against the numpy model
(tests/position_nonlinear_model.py) on the inputs of tests/position_nonlinear_cases.py.

tests/test_position_nonlinear_cpu.py holds the model, on these same inputs, to a smallest decision margin above 1e-6, so
the trajectory -- every step's outcome, the iteration count, the termination -- is compared with equality.  The start is
compared bit for bit (it is integer arithmetic and three roundings).  The cost and radius traces and the positions are
compared at the relative tolerance of the project's device-versus-oracle parity tests, 1e-9: the factorisation's
summation order is not numpy's.  For the positions the measure is max |device - model| over the largest |model position|
-- the problem fixes one view and no scale, so a view near the origin has no relative accuracy of its own.
Shapes: orders 3, 9, 21, 33, 117, 207 (more than three 64-column panels, a chain) and 900; a star whose hub row (300
edges) is longer than a workgroup; the fixed view first, in the middle and last; the small-norm branch from a given start;
0 and 1 iterations."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402
import position_nonlinear_cases as cases  # noqa: E402
import position_nonlinear_model as model  # noqa: E402
from theiasfm_amd import abi, lib  # noqa: E402

pytestmark = pytest.mark.gpu
RTOL = 1e-9


@pytest.fixture(scope="module")
def L():
    entry.build_engine()
    return lib.load()


def _device(case, pre_rotated=False):
    o, v1, v2, p2 = case["view_rotation"], case["view1"], case["view2"], case["position2"]
    if pre_rotated:
        batch = abi.ViewPairBatch(None, v1, v2, None, model.directions(o, v1, p2), o.shape[0])
    else:
        batch = abi.ViewPairBatch(o, v1, v2, None, p2)
    return lib.estimate_global_positions_nonlinear(batch, case["fixed_view"],
                                                   abi.nonlinear_position_options(**case["options"]), start=case["start"])


def _compare(name, case, dev, base):
    s = dev["summary"]
    scale = float(np.abs(base["positions"]).max())
    diff = float(np.abs(dev["positions"] - base["positions"]).max()) / scale
    print("%s: %d iterations (model %d), termination %d (model %d), outcomes %s, positions differ by %.3e of %.3e, "
          "final cost %.6e" % (name, s.num_iterations, base["iterations"], s.termination, base["termination"],
                               dev["outcomes"].tolist(), diff, scale, s.final_cost))
    assert dev["initial_positions"].tobytes() == base["initial_positions"].tobytes()
    assert dev["outcomes"].tolist() == base["outcomes"].tolist()
    assert (s.num_iterations, s.termination) == (base["iterations"], base["termination"])
    assert bool(s.usable) and s.num_factorizations == base["factorizations"]
    assert s.num_successful_steps == int((base["outcomes"][1:] == 1).sum())
    assert s.num_unsuccessful_steps == int((base["outcomes"][1:] <= 0).sum())
    assert (s.num_views, s.num_pairs) == (case["view_rotation"].shape[0], case["view1"].size)
    # cost = |r|^2 / 2 with r a vector of differences of unit vectors: where the solve drives it towards 0 (the
    # noise-free scenes end near 1e-21) r is all cancellation and the cost has no relative accuracy left.  The absolute
    # term is what the tolerance on the positions already grants: |d cost| = |r . dr| <= sqrt(2 cost) |dr| with every
    # entry of dr within RTOL, |dr| <= RTOL sqrt(3 E).  At the start (cost of order 1) it is of the size of the
    # relative term.
    floor = RTOL * np.sqrt(2.0 * base["costs"] * 3.0 * case["view1"].size)
    allowed = RTOL * np.abs(base["costs"]) + floor
    off = np.abs(dev["costs"] - base["costs"])
    print("%s: largest |cost difference| / allowed %.3e, largest relative cost difference %.3e" %
          (name, float((off / np.maximum(allowed, 1e-300)).max()), float((off / np.maximum(base["costs"], 1e-300)).max())))
    assert (off <= allowed).all()
    np.testing.assert_allclose(dev["radii"], base["radii"], rtol=RTOL)
    assert (s.initial_cost, s.final_cost) == (dev["costs"][0], dev["costs"][-1])
    assert diff <= RTOL
    np.testing.assert_allclose(dev["residuals"], base["residuals"], rtol=0.0, atol=RTOL * 2.0)  # |r| <= 2
    assert (dev["positions"][case["fixed_view"]] == 0.0).all()
    if s.num_iterations:
        assert s.kernel_seconds > 0 and s.seconds >= s.kernel_seconds
        assert s.kernel_seconds == pytest.approx(s.factor_seconds + s.substitution_seconds + s.graph_seconds)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_device_equals_model(L, name):
    case, base = cases.expected(name)
    dev = _device(case)
    _compare(name, case, dev, base)
    if name in cases.REFERENCE_BOUND:  # the reference's own tests, after alignment to the ground truth
        err = float((model.aligned_errors(case["gt"], dev["positions"]) ** 2).max())
        print("%s: largest squared error after alignment on the device %.3e" % (name, err))
        assert err < cases.REFERENCE_BOUND[name]


@pytest.mark.parametrize("name", cases.PRE_ROTATED)
def test_pre_rotated_directions_without_view_rotation(L, name):
    """view_rotation NULL with the model's t_e as position_2: the same problem without the direction kernel."""
    case, base = cases.expected(name)
    _compare(name + " (pre-rotated)", case, _device(case, pre_rotated=True), base)


def test_two_calls_give_the_same_bytes(L):
    for name in ("random 40/200, a fifth outliers", "star of 300, leaf fixed", "shuffled path of 70"):
        case = cases.expected(name)[0]
        a, b = _device(case), _device(case)
        for key in ("positions", "initial_positions", "residuals", "costs", "radii", "outcomes"):
            assert a[key].tobytes() == b[key].tobytes(), (name, key)


def test_a_given_start_is_not_overwritten_on_failure_and_is_on_success(L, monkeypatch):
    case = cases.expected("coincident start")[0]
    o, v1, v2, p2 = case["view_rotation"], case["view1"], case["view2"], case["position2"]
    batch = abi.ViewPairBatch(o, v1, v2, None, p2)
    cb = batch.as_c()
    opt = abi.nonlinear_position_options(positions_given=1)
    s = abi.CNonlinearPositionSummary()
    pos = case["start"].copy()
    monkeypatch.setenv("TMI_BA_ROTATION_MAX_ORDER", "3")
    rc = L.tmi_ba_estimate_global_positions_nonlinear(C.byref(cb), C.byref(opt), 0, -1, pos.ctypes.data, None, None, None,
                                                      None, None, C.byref(s))
    assert rc == 5 and pos.tobytes() == case["start"].tobytes()
    monkeypatch.delenv("TMI_BA_ROTATION_MAX_ORDER")
    rc = L.tmi_ba_estimate_global_positions_nonlinear(C.byref(cb), C.byref(opt), 0, -1, pos.ctypes.data, None, None, None,
                                                      None, None, C.byref(s))  # every optional output NULL
    assert rc == 0 and s.usable and (pos[0] == 0.0).all()
    assert pos.tobytes() == _device(case)["positions"].tobytes()
