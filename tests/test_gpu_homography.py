"""tmi_ba_estimate_homographies on the device against its numpy model (tests/homography_model.py) on the inputs of
tests/homography_cases.py, under both scorings: 12 pairs of 3, 4, 5, 63, 64, 65, 130 and five of 40-200 correspondences
with min_iterations 16 and max_iterations 64, three pairs with planted samples and the reference's own lattice scene.

The integer outputs must be EQUAL to the model's wherever the model's decision margins (homography_model.py) are at
least 1e-9 -- tests/test_homography_cpu.py checks on exactly these inputs that at most 2 % of the replayed hypotheses are
flagged and that none of them is a best model or changes a bound.  The MLE costs must be BITWISE equal to the model's
scalar path (the sum has one fixed shape).  The homography (unit Frobenius norm, largest entry positive) and the
confidence must agree within max(1e-12, 100 x MODEL_SPREAD), MODEL_SPREAD the difference between the model's two paths on
the same input."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import homography_cases as cases  # noqa: E402
import homography_model as model  # noqa: E402
from theiasfm_amd import abi, lib  # noqa: E402

pytestmark = pytest.mark.gpu
INTS = ("status", "num_correspondences", "num_inliers", "num_iterations", "best_iteration", "corr_inlier")
SCORINGS = [False, True]


def _options(use_mle, **kw):
    return abi.homography_ransac_options(min_iterations=cases.MIN_ITERATIONS, max_iterations=cases.MAX_ITERATIONS,
                                         device=0, use_mle=int(use_mle), **kw)


def _run_main(use_mle, chunk=0, pair_mask=None):
    b = cases.main_batch()
    return lib.estimate_homographies(
        b["pair_offset"], b["feature1"], b["feature2"], np.full(len(cases.MAIN_COUNTS), cases.THRESHOLD),
        options=_options(use_mle, seed=cases.MAIN_RANSAC_SEED, chunk_iterations=chunk), pair_mask=pair_mask,
        want_hypothesis_cost=True, want_hypothesis_cost_real=use_mle)


@pytest.fixture(scope="module")
def main_device():
    return {use_mle: _run_main(use_mle) for use_mle in SCORINGS}


def _assert_equal_to_model(dev, ref, use_mle):
    for k in INTS:
        assert np.array_equal(dev[k], ref[k]), k
    keep = ~ref["flagged"]
    assert np.array_equal(dev["hypothesis_cost"][keep], ref["hypothesis_cost"][keep])
    if use_mle:
        # bit for bit, NaN (no model, not replayed) included
        assert dev["hypothesis_cost_real"][keep].tobytes() == ref["hypothesis_cost_real"][keep].tobytes()
        assert np.array_equal(np.isnan(dev["hypothesis_cost_real"]), dev["hypothesis_cost"] < 0)
    else:
        assert dev["hypothesis_cost_real"] is None


def _assert_reals(dev, ref, ref_numpy, what):
    spread = model.model_spread(ref, ref_numpy)
    tol = max(1e-12, 100.0 * spread)
    ok = ref["status"] == 0
    worst = max(np.abs(model.unit_h(dev["homography"][ok]) - model.unit_h(ref["homography"][ok])).max(),
                np.abs(dev["confidence"][ok] - ref["confidence"][ok]).max())
    print(f"{what}: MODEL_SPREAD {spread:.3e} tolerance {tol:.3e} device-model worst {worst:.3e} ratio {worst / tol:.3e}")
    assert worst <= tol
    assert (dev["homography"][~ok] == 0.0).all()


@pytest.mark.parametrize("use_mle", SCORINGS)
def test_device_against_model(main_device, use_mle):
    dev, ref = main_device[use_mle], cases.main_model(use_mle)
    _assert_equal_to_model(dev, ref, use_mle)
    _assert_reals(dev, ref, cases.main_model(use_mle, "numpy"), f"main use_mle={use_mle}")
    s = dev["summary"]
    assert (s.num_pairs, s.num_too_few_correspondences) == (12, 1)
    assert s.num_estimated == int(np.count_nonzero(ref["status"] == 0))
    assert s.num_no_model == int(np.count_nonzero(ref["status"] == 2))
    assert s.total_iterations == int(ref["num_iterations"].sum())


def test_the_two_scorings_differ(main_device):
    """The MLE path is taken: on cases.MLE_PAIR the model's two scorings pick different best iterations
    (tests/test_homography_cpu.py), and so does the device."""
    p = cases.MLE_PAIR
    assert main_device[False]["best_iteration"][p] != main_device[True]["best_iteration"][p]
    assert main_device[True]["best_iteration"][p] == cases.main_model(True)["best_iteration"][p]


@pytest.mark.parametrize("use_mle", SCORINGS)
def test_result_does_not_depend_on_the_chunking_or_the_run(main_device, use_mle):
    keys = INTS + ("confidence", "homography", "hypothesis_cost") + (("hypothesis_cost_real",) if use_mle else ())
    for chunk in (0, 5, 64):  # (0 again: a repeated call gives the same bytes)
        other = _run_main(use_mle, chunk)
        for k in keys:
            assert main_device[use_mle][k].tobytes() == other[k].tobytes(), (chunk, k)
        if chunk == 5:
            assert other["summary"].num_chunks > main_device[use_mle]["summary"].num_chunks


@pytest.mark.parametrize("use_mle", SCORINGS)
def test_planted_samples(use_mle):
    b = cases.planted_batch()
    ref = cases.planted_model(use_mle)
    dev = lib.estimate_homographies(b["pair_offset"], b["feature1"], b["feature2"], np.full(3, cases.THRESHOLD),
                                    options=_options(use_mle), samples=b["samples"], want_hypothesis_cost=True,
                                    want_hypothesis_cost_real=use_mle)
    _assert_equal_to_model(dev, ref, use_mle)
    # three collinear points, a repeated correspondence: rank < 8, no model, and the iteration counts
    for p in (0, 1):
        assert ref["results"][p].hyp[0].reason == "rank" and dev["hypothesis_cost"][p, 0] == -1
        assert dev["status"][p] == 0 and dev["num_iterations"][p] >= 1
    # every sample degenerate
    assert dev["status"][2] == 2 and dev["num_inliers"][2] == 0 and dev["best_iteration"][2] == -1
    assert (dev["hypothesis_cost"][2] == -1).all() and dev["num_iterations"][2] == cases.MAX_ITERATIONS
    assert (dev["homography"][2] == 0.0).all() and dev["summary"].num_no_model == 1
    # a repeated index is an argument error
    bad = b["samples"].copy()
    bad[0, 3, 3] = bad[0, 3, 2]
    with pytest.raises(lib.EngineError) as e:
        lib.estimate_homographies(b["pair_offset"], b["feature1"], b["feature2"], np.full(3, cases.THRESHOLD),
                                  options=_options(use_mle), samples=bad)
    assert e.value.status == abi.ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("use_mle", SCORINGS)
def test_mask_and_empty_batch(main_device, use_mle):
    full = main_device[use_mle]
    mask = np.zeros(len(cases.MAIN_COUNTS), dtype=np.uint8)
    mask[[4, 9]] = 1
    part = _run_main(use_mle, pair_mask=mask)
    assert (part["status"][mask == 0] == -1).all() and part["summary"].num_pairs == 2
    po = cases.main_batch()["pair_offset"]
    for p in (4, 9):
        for k in INTS[:5] + ("confidence", "homography"):
            assert part[k][p].tobytes() == full[k][p].tobytes(), (p, k)
        assert np.array_equal(part["corr_inlier"][po[p]:po[p + 1]], full["corr_inlier"][po[p]:po[p + 1]])
    assert np.array_equal(part["hypothesis_cost"], full["hypothesis_cost"][[4, 9]])  # (rows: selected pairs)
    if use_mle:
        assert part["hypothesis_cost_real"].tobytes() == full["hypothesis_cost_real"][[4, 9]].tobytes()
    assert part["corr_inlier"].sum() == full["corr_inlier"][po[4]:po[5]].sum() + full["corr_inlier"][po[9]:po[10]].sum()
    empty = lib.estimate_homographies(np.zeros(1, np.int64), np.zeros((0, 2)), np.zeros((0, 2)), np.zeros(0),
                                      options=_options(use_mle))
    assert empty["status"].shape == (0,) and empty["summary"].num_pairs == 0


def test_reference_scene_with_mle():
    """estimate_homography_test.cc:65-128 with use_mle, as all four of the reference's tests set it: success, more than 4
    inliers, and all 81 in the noise-free all-inlier variant; the device equals the model here too."""
    b = cases.reference_batch()
    ref = cases.reference_model()
    kw = dict(cases.REFERENCE_KW)
    dev = lib.estimate_homographies(b["pair_offset"], b["feature1"], b["feature2"],
                                    np.full(24, cases.REFERENCE_THRESHOLD),
                                    options=abi.homography_ransac_options(device=0, seed=cases.REFERENCE_RANSAC_SEED,
                                                                          failure_probability=kw["failure_probability"],
                                                                          min_iterations=kw["min_iterations"],
                                                                          max_iterations=kw["max_iterations"], use_mle=1),
                                    want_hypothesis_cost=True, want_hypothesis_cost_real=True)
    assert (dev["status"] == 0).all() and (dev["num_inliers"] > 4).all() and (dev["num_inliers"][:6] == 81).all()
    _assert_equal_to_model(dev, ref, True)
