"""tmi_ba_estimate_positions_known_orientation and tmi_ba_estimate_relative_positions_known_orientation on the device
against their numpy model (tests/known_orientation_model.py) on the inputs of tests/known_orientation_cases.py, under
both scorings: ten items of 2, 3, 63, 64, 65, 130 correspondences, one of 1 (status 1), a masked one, a degenerate one
(status 2) and one with 40 % gross outliers, min_iterations 16 and max_iterations 64; three items with planted samples;
the reference's own scenes.

The rotation (step 2) calls the device's sin and cos, the model the C library's.  So the rotated features the device
returns are checked against the model's rotation within ROTATION_TOLERANCE, and everything after them -- a function of
the rotated features in + - * / sqrt -- against the model run ON THE DEVICE'S ROTATED FEATURES, where it must be EQUAL:
every integer output, hypothesis_cost, the position's bytes, and hypothesis_cost_real byte for byte on the hypotheses
the model does not flag (decision margins below 1e-9, known_orientation_model.py).  At most 1 % of the replayed
hypotheses may be flagged; tests/test_known_orientation_cpu.py checks the same on the model's own rotation."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import known_orientation_cases as cases  # noqa: E402
import known_orientation_model as model  # noqa: E402
from theiasfm_amd import abi, lib  # noqa: E402

pytestmark = pytest.mark.gpu
INTS = ("status", "num_correspondences", "num_inliers", "num_iterations", "best_iteration", "corr_inlier")
SCORINGS = [False, True]
BOTH = [(kind, use_mle) for kind in cases.KINDS for use_mle in SCORINGS]
# sin and cos within 2 ulp each, an entry of R three more roundings on magnitudes <= 1 (6 eps), a ray coordinate three
# such terms and three roundings (21 eps), the quotient of two of them on |values| <= 1.2 with ray_2 >= 0.9: below
# 64 eps, whether or not the rotation matrix' expressions are contracted
ROTATION_TOLERANCE = 64 * model.EPS
MAX_FLAGGED_SHARE = 0.01


def _options(use_mle, **kw):
    kw.setdefault("min_iterations", cases.MIN_ITERATIONS)
    kw.setdefault("max_iterations", cases.MAX_ITERATIONS)
    return abi.known_orientation_ransac_options(device=0, use_mle=int(use_mle), **kw)


def _rotated(dev):
    return [dev[k] for k in ("rotated_feature", "rotated_feature1", "rotated_feature2") if k in dev]


def _call(b, thresholds, options, **kw):
    if b["kind"] == "absolute":
        return lib.estimate_positions_known_orientation(b["item_offset"], b["features"][0], b["world_point"],
                                                        b["orientations"][0], thresholds, options=options, **kw)
    if "item_mask" in kw:
        kw["pair_mask"] = kw.pop("item_mask")
    return lib.estimate_relative_positions_known_orientation(b["item_offset"], b["features"][0], b["features"][1],
                                                             b["orientations"][0], b["orientations"][1], thresholds,
                                                             options=options, **kw)


def _run_main(kind, use_mle, chunk=0, mask=cases.MAIN_MASK):
    return _call(cases.main_batch(kind), np.full(len(cases.MAIN_COUNTS), cases.THRESHOLD),
                 _options(use_mle, seed=cases.MAIN_RANSAC_SEED, chunk_iterations=chunk), item_mask=mask,
                 want_hypothesis_cost=True, want_hypothesis_cost_real=use_mle)


@pytest.fixture(scope="module")
def main_device():
    return {key: _run_main(*key) for key in BOTH}


@pytest.fixture(scope="module")
def main_reference(main_device):
    """The model on the device's rotated features, once per (kind, scoring)."""
    return {(kind, use_mle): cases.run_model(cases.main_batch(kind), np.full(len(cases.MAIN_COUNTS), cases.THRESHOLD),
                                             rotated=_rotated(main_device[kind, use_mle]), item_mask=cases.MAIN_MASK,
                                             seed=cases.MAIN_RANSAC_SEED, use_mle=use_mle, **cases.KW)
            for kind, use_mle in BOTH}


def _assert_equal_to_model(dev, ref, use_mle):
    for k in INTS:
        assert np.array_equal(dev[k], ref[k]), k
    assert np.array_equal(dev["hypothesis_cost"], ref["hypothesis_cost"])
    replayed = ref["hypothesis_cost"] >= 0
    share = np.count_nonzero(ref["flagged"]) / max(int(np.count_nonzero(replayed)), 1)
    print(f"flagged {np.count_nonzero(ref['flagged'])} of {np.count_nonzero(replayed)} hypotheses with a model")
    assert share <= MAX_FLAGGED_SHARE
    keep = ~ref["flagged"]
    if use_mle:
        # byte for byte, NaN (no model, not replayed) included
        assert dev["hypothesis_cost_real"][keep].tobytes() == ref["hypothesis_cost_real"][keep].tobytes()
        assert np.array_equal(np.isnan(dev["hypothesis_cost_real"]), dev["hypothesis_cost"] < 0)
    else:
        assert dev["hypothesis_cost_real"] is None
    assert dev["position"].tobytes() == ref["position"].tobytes()
    assert np.abs(dev["confidence"] - ref["confidence"]).max() <= 1e-12


def _assert_rotation(dev, own):
    for d, m in zip(_rotated(dev), own["rotated"]):
        worst = float(np.abs(d - m).max())
        print(f"rotated features: device - model worst {worst:.3e}, tolerance {ROTATION_TOLERANCE:.3e}")
        assert worst <= ROTATION_TOLERANCE


@pytest.mark.parametrize("kind,use_mle", BOTH)
def test_device_against_model(main_device, main_reference, kind, use_mle):
    dev, ref = main_device[kind, use_mle], main_reference[kind, use_mle]
    _assert_rotation(dev, cases.main_model(kind, use_mle))
    _assert_equal_to_model(dev, ref, use_mle)
    assert dev["status"].tolist() == [0, 0, 0, 0, 0, 0, 1, -1, 2, 0]
    # the degenerate item: every sample without a model, every iteration run
    p, row = cases.DEGENERATE_ITEM, cases.DEGENERATE_ITEM - 1  # (rows: selected items; item 7 is masked)
    assert (dev["hypothesis_cost"][row] == -1).all() and dev["num_iterations"][p] == cases.MAX_ITERATIONS
    assert (dev["position"][[cases.STATUS1_ITEM, cases.MASKED_ITEM, p]] == 0.0).all()
    # the truth is found in spite of 40 % gross outliers (the bound of the reference's outlier tests)
    q = cases.OUTLIER_ITEM
    assert model.direction_difference(dev["position"][q], cases.main_batch(kind)["position"][q]) <= 1e-2
    if kind == "relative":
        ok = dev["status"] == 0
        assert np.abs(np.linalg.norm(dev["position"][ok], axis=1) - 1.0).max() <= 4 * model.EPS
    s = dev["summary"]
    assert (s.num_pairs, s.num_too_few_correspondences, s.num_estimated, s.num_no_model) == (9, 1, 7, 1)
    assert s.total_iterations == int(ref["num_iterations"].sum())


@pytest.mark.parametrize("kind", cases.KINDS)
def test_the_two_scorings_differ(main_device, main_reference, kind):
    """The MLE path is taken: on cases.MLE_ITEM the model's two scorings pick different best iterations
    (tests/test_known_orientation_cpu.py), and so does the device."""
    p = cases.MLE_ITEM[kind]
    assert main_device[kind, False]["best_iteration"][p] != main_device[kind, True]["best_iteration"][p]
    assert main_device[kind, True]["best_iteration"][p] == main_reference[kind, True]["best_iteration"][p]


@pytest.mark.parametrize("kind,use_mle", BOTH)
def test_result_does_not_depend_on_the_chunking_or_the_run(main_device, kind, use_mle):
    keys = INTS + ("confidence", "position", "hypothesis_cost") + (("hypothesis_cost_real",) if use_mle else ())
    first = main_device[kind, use_mle]
    for chunk in (0, 1, 7):  # (0 again: a repeated call gives the same bytes)
        other = _run_main(kind, use_mle, chunk)
        for k in keys:
            assert first[k].tobytes() == other[k].tobytes(), (chunk, k)
        for a, b in zip(_rotated(first), _rotated(other)):
            assert a.tobytes() == b.tobytes()
        if chunk:
            assert other["summary"].num_chunks > first["summary"].num_chunks


@pytest.mark.parametrize("kind,use_mle", BOTH)
def test_planted_samples(kind, use_mle):
    b = cases.planted_batch(kind)
    th = np.full(3, cases.THRESHOLD)
    dev = _call(b, th, _options(use_mle), samples=b["samples"], want_hypothesis_cost=True,
                want_hypothesis_cost_real=use_mle)
    ref = cases.run_model(b, th, rotated=_rotated(dev), samples=b["samples"], use_mle=use_mle, **cases.KW)
    _assert_equal_to_model(dev, ref, use_mle)
    # a sample of a correspondence and its copy: rank deficient, no model, and it counts as an iteration
    assert ref["results"][0].hyp[0].reason == "rank" and dev["hypothesis_cost"][0, 0] == -1
    assert dev["status"][0] == 0 and dev["num_iterations"][0] >= 1 and dev["best_iteration"][0] >= 1
    # every sample degenerate
    assert dev["status"][2] == 2 and dev["num_inliers"][2] == 0 and dev["best_iteration"][2] == -1
    assert (dev["hypothesis_cost"][2] == -1).all() and dev["num_iterations"][2] == cases.MAX_ITERATIONS
    assert dev["summary"].num_no_model == 1
    # a repeated or out-of-range index is an argument error
    for wrong in ((3, 3), (0, 30), (-1, 2)):
        bad = b["samples"].copy()
        bad[0, 3] = wrong
        with pytest.raises(lib.EngineError) as e:
            _call(b, th, _options(use_mle), samples=bad)
        assert e.value.status == abi.ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("kind", cases.KINDS)
def test_mask_and_empty_batch(main_device, kind):
    full = main_device[kind, True]
    assert full["hypothesis_cost"].shape == (9, cases.MAX_ITERATIONS)  # (rows: selected items)
    mask = np.zeros(len(cases.MAIN_COUNTS), dtype=np.uint8)
    mask[[4, 9]] = 1
    part = _run_main(kind, True, mask=mask)
    assert (part["status"][mask == 0] == -1).all() and part["summary"].num_pairs == 2
    po = cases.main_batch(kind)["item_offset"]
    for p in (4, 9):
        for k in INTS[:5] + ("confidence", "position"):
            assert part[k][p].tobytes() == full[k][p].tobytes(), (p, k)
        assert np.array_equal(part["corr_inlier"][po[p]:po[p + 1]], full["corr_inlier"][po[p]:po[p + 1]])
    assert np.array_equal(part["hypothesis_cost"], full["hypothesis_cost"][[4, 8]])
    assert part["hypothesis_cost_real"].tobytes() == full["hypothesis_cost_real"][[4, 8]].tobytes()
    empty = dict(kind=kind, item_offset=np.zeros(1, np.int64), features=[np.zeros((0, 2))] * 2,
                 orientations=[np.zeros((0, 3))] * 2, world_point=np.zeros((0, 3)))
    out = _call(empty, np.zeros(0), _options(True))
    assert out["status"].shape == (0,) and out["summary"].num_pairs == 0
    none = _run_main(kind, True, mask=np.zeros(len(cases.MAIN_COUNTS), dtype=np.uint8))
    assert (none["status"] == -1).all() and none["summary"].num_pairs == 0


@pytest.mark.parametrize("kind", cases.KINDS)
def test_reference_scenes_with_mle(kind):
    """The reference's four estimator tests per call with use_mle, as all eight set it: success, more than 3 inliers,
    the position (direction) within the test's tolerance in ArraysEqualUpToScale's measure; the device equals the
    model here too."""
    b = cases.reference_batch(kind)
    th = np.full(len(b["tolerance"]), cases.REFERENCE_THRESHOLD)
    kw = dict(cases.REFERENCE_KW)
    kw.pop("use_mle")
    dev = _call(b, th, _options(True, seed=cases.REFERENCE_RANSAC_SEED, **kw), want_hypothesis_cost=True,
                want_hypothesis_cost_real=True)
    assert (dev["status"] == 0).all() and (dev["num_inliers"] > 3).all()
    for p, tol in enumerate(b["tolerance"]):
        assert model.direction_difference(dev["position"][p], b["position"][p]) <= tol, p
    _assert_rotation(dev, cases.reference_model(kind))
    ref = cases.run_model(b, th, rotated=_rotated(dev), seed=cases.REFERENCE_RANSAC_SEED, **cases.REFERENCE_KW)
    _assert_equal_to_model(dev, ref, True)
