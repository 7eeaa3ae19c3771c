"""-m gpu: tmi_ba_estimate_global_positions_linear against its numpy restatement (tests/position_linear_model.py) on the
shared case list (tests/position_linear_cases.py).

Integers (triplets, pair indices, common and used counts, components, view_estimated, the iteration count, sign_votes)
must be equal.  Baselines: 1e-9 relative, what tests/test_gpu_estimate_tracks.py holds triangulated points to (the same
arithmetic; the case generator asserts that no ray pair lies within 1e-9 of the angle threshold).  Positions: within
model.derived_bound(C, ...) of the model's, C = 4 -- the largest ratio of |model - plain| to the bound with c = 1 over
the case list is 0.115 (model_fisheye), measured by test_position_linear_cpu.py::test_comparison_bound.  The one case
with a double smallest eigenvalue (one triplet alone) has no bound of that form: there the device's vector is held to
its eigen-residual against the model's matrix."""
import numpy as np
import pytest

import position_linear_cases as cases
import position_linear_model as model
from theiasfm_amd import abi, lib

pytestmark = pytest.mark.gpu

BOUND_C = 4.0
TRIPLET_KEYS = ("triplet_view", "triplet_pair", "triplet_num_common", "triplet_num_used", "triplet_component")


def run(name, **kw):
    c = cases.case(name)
    return lib.estimate_global_positions_linear(c["P"], c["batch"], abi.linear_position_options(**c["options"]), **kw)


@pytest.mark.parametrize("name", cases.NAMES)
def test_matches_model(name):
    c = cases.case(name)
    ref, plain = cases.reference(name)
    out = run(name)
    s = out["summary"]
    print(name, "triplets", s.num_triplets, "order", s.order, "iterations", s.num_iterations, ref["iterations"],
          "residual", s.residual, "votes", s.sign_votes, ref["sign_votes"])
    for key in TRIPLET_KEYS:
        np.testing.assert_array_equal(out[key], ref[key], err_msg=key)
    np.testing.assert_allclose(out["triplet_baseline"], ref["triplet_baseline"], rtol=1e-9, atol=0.0)
    np.testing.assert_array_equal(out["estimated"], ref["estimated"])
    assert (s.num_views, s.num_pairs) == (c["batch"].num_views, c["batch"].num_pairs)
    assert s.num_triplets == len(ref["triplet_view"])
    assert s.num_triplets_with_baseline == int((ref["triplet_num_used"] > 0).sum())
    assert s.num_triplet_components == ref["num_components"]
    assert s.num_chosen_triplets == len(ref["chosen"])
    assert s.num_chosen_views == len(ref["views"])
    assert s.num_dropped_ratios == ref["num_dropped"]
    assert (s.usable, s.order, s.converged) == (ref["usable"], ref["order"], ref["converged"])
    assert ref["stop_margin"] > 1e-3  # (the model's last residuals are not at the threshold: the count is well defined)
    assert s.num_iterations == ref["iterations"]
    # the vote kernel against the model's vote on the DEVICE's own vector (before the flip), in every case ...
    unflipped = out["positions"] * (-1.0 if s.flipped else 1.0)
    assert s.sign_votes == model.sign_votes(c["batch"], unflipped, ref["estimated"])
    assert s.flipped == int(s.sign_votes < 0)
    # ... and against the model's own, except where any vector of an eigen-plane is an answer and the vote follows it
    if name not in cases.DEGENERATE:
        assert s.sign_votes == ref["sign_votes"] and s.flipped == ref["flipped"]
    np.testing.assert_allclose(s.matrix_norm, ref["matrix_norm"], rtol=1e-9)
    free = np.array(ref["views"][1:])
    x = out["positions"][free].ravel() * (-1.0 if s.flipped else 1.0)
    assert abs(np.linalg.norm(x) - 1.0) < 1e-12
    np.testing.assert_array_equal(out["positions"][ref["estimated"] == 0], 0.0)
    threshold = ref["options"]["tolerance"] * ref["matrix_norm"]
    residual = np.linalg.norm(ref["M"] @ x - (x @ ref["M"] @ x) * x)
    print(name, "eigen-residual", residual, "threshold", threshold)
    assert residual <= 2.0 * threshold
    if name in cases.DEGENERATE:
        return
    w = plain["eigenvalues"]
    bound = model.derived_bound(BOUND_C, ref["order"], ref["options"]["tolerance"], ref["matrix_norm"], w[1] - w[0])
    distance = np.linalg.norm(out["positions"] - ref["positions"])
    print(name, "distance", distance, "bound", bound)
    assert bound <= 1e-6
    assert distance <= bound


@pytest.mark.parametrize("name", ["four_noisy", "wheel", "tracks_1025", "dropped_changes_choice"])
def test_two_calls_same_bytes(name):
    a, b = run(name, triplet_capacity=128), run(name, triplet_capacity=128)  # (one call each: the capacity is given)
    for key in ("positions", "estimated", "triplet_baseline") + TRIPLET_KEYS:
        assert a[key].tobytes() == b[key].tobytes(), key
    for f in ("num_iterations", "residual", "sign_votes", "matrix_norm"):
        assert getattr(a["summary"], f) == getattr(b["summary"], f)
    assert list(a["summary"].eigenvalue) == list(b["summary"].eigenvalue)


def _sentinel_call(P, batch, options, capacity):
    V = batch.num_views
    pos, est = np.full((V, 3), 7.25), np.full(V, 9, dtype=np.uint8)
    out = lib.estimate_global_positions_linear(P, batch, options, triplet_capacity=capacity, view_position=pos,
                                               view_estimated=est)
    return out, pos, est


def test_unusable_writes_nothing():
    """No triangle at all, and a graph whose only triplet has no common track: TMI_BA_OK, usable = 0, sentinels intact."""
    c = cases.case("no_common_track")
    for pairs in ([(0, 1), (0, 2), (1, 3)], [(4, 5), (4, 6), (5, 6)]):
        keep = [i for i, p in enumerate(zip(c["batch"].pair_view1, c["batch"].pair_view2)) if tuple(map(int, p)) in pairs]
        b = c["batch"]
        sub = abi.ViewPairBatch(b.view_rotation, b.pair_view1[keep], b.pair_view2[keep], b.pair_rotation2[keep],
                                b.pair_position2[keep])
        assert sub.num_pairs == 3
        out, pos, est = _sentinel_call(c["P"], sub, None, 4)
        assert out["summary"].usable == 0
        np.testing.assert_array_equal(out["positions"], pos)
        np.testing.assert_array_equal(out["estimated"], est)
        assert out["triplet_view"] is None or not out["summary"].triplets_written


def test_zero_shift_on_the_singular_case():
    """relative_shift = 0 on the noise-free problem: M is singular to rounding.  Whether a pivot comes out positive is
    rounding's choice; either nothing is written, or the answer is the plain one."""
    c = cases.case("four_clean")
    _, plain = cases.reference("four_clean")
    out, pos, est = _sentinel_call(c["P"], c["batch"], abi.linear_position_options(relative_shift=0.0), 0)
    s = out["summary"]
    print("zero shift: usable", s.usable, "iterations", s.num_iterations, "residual", s.residual)
    if not s.usable:
        np.testing.assert_array_equal(out["positions"], pos)
        np.testing.assert_array_equal(out["estimated"], est)
    else:
        assert s.converged
        errors = model.umeyama_errors(out["positions"], c["truth"])
        assert errors.max() < 1e-4
        assert np.linalg.norm(out["positions"] - plain["positions"]) < 1e-6


def test_small_capacity_still_solves():
    full = run("two_and_one")
    small = run("two_and_one", triplet_capacity=2)
    assert small["summary"].num_triplets == 3 and not small["summary"].triplets_written
    assert small["triplet_view"] is None
    assert small["positions"].tobytes() == full["positions"].tobytes()


def test_order_cap_is_unsupported(monkeypatch):
    """TMI_BA_ROTATION_MAX_ORDER (read per call) below the order 9: TMI_BA_ERR_UNSUPPORTED and nothing written."""
    c = cases.case("four_noisy")
    monkeypatch.setenv("TMI_BA_ROTATION_MAX_ORDER", "8")
    with pytest.raises(lib.EngineError) as err:
        lib.estimate_global_positions_linear(c["P"], c["batch"], triplet_capacity=0)
    assert err.value.status == abi.ERR_UNSUPPORTED
    monkeypatch.setenv("TMI_BA_ROTATION_MAX_ORDER", "9")
    assert lib.estimate_global_positions_linear(c["P"], c["batch"], triplet_capacity=0)["summary"].usable == 1
