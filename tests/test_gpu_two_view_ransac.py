"""tmi_ba_estimate_uncalibrated_relative_poses on the device against its numpy model (tests/two_view_ransac_model.py) on
the inputs of tests/two_view_ransac_cases.py: 12 pairs of 7, 8, 9, 63, 64, 65, 130 and five of 40-200 correspondences
with min_iterations 16 and max_iterations 64, and three pairs with planted samples.

The integer outputs must be EQUAL to the model's wherever the model's decision margins (two_view_ransac_model.py) are at
least 1e-9 -- tests/test_two_view_ransac_cpu.py checks on exactly these inputs that at most 2 % of the replayed
hypotheses are flagged and that none of them is a best model or changes a bound.  The real-valued outputs must agree
within max(1e-12, 100 x MODEL_SPREAD), MODEL_SPREAD the difference between the model's two paths on the same input."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import two_view_ransac_cases as cases  # noqa: E402
import two_view_ransac_model as model  # noqa: E402
from theiasfm_amd import abi, lib, synth  # noqa: E402

pytestmark = pytest.mark.gpu
INTS = ("status", "num_correspondences", "num_inliers", "num_iterations", "best_iteration", "corr_inlier")
REALS = ("focal_length1", "focal_length2", "rotation", "position", "confidence")


def _options(**kw):
    return abi.two_view_ransac_options(min_iterations=cases.MIN_ITERATIONS, max_iterations=cases.MAX_ITERATIONS,
                                       device=0, **kw)


def _run_main(chunk=0, pair_mask=None):
    b = cases.main_batch()
    return lib.estimate_uncalibrated_relative_poses(
        b["pair_offset"], b["feature1"], b["feature2"], np.full(len(cases.MAIN_COUNTS), cases.THRESHOLD),
        options=_options(seed=cases.MAIN_RANSAC_SEED, chunk_iterations=chunk), pair_mask=pair_mask,
        want_hypothesis_cost=True)


@pytest.fixture(scope="module")
def main_device():
    return _run_main()


def _assert_equal_to_model(dev, ref):
    for k in INTS:
        assert np.array_equal(dev[k], ref[k]), k
    keep = ~ref["flagged"]
    assert np.array_equal(dev["hypothesis_cost"][keep], ref["hypothesis_cost"][keep])


def test_device_against_model(main_device):
    ref = cases.main_model()
    _assert_equal_to_model(main_device, ref)
    assert sorted(set(ref["status"].tolist())) == [0, 1, 2]  # the inputs cover every status
    spread = model.model_spread(ref, cases.main_model("numpy"))
    tol = max(1e-12, 100.0 * spread)
    ok = ref["status"] == 0
    worst = np.abs(model.unit_f(main_device["fundamental_matrix"][ok]) - model.unit_f(ref["fundamental_matrix"][ok])).max()
    for k in REALS:
        scale = np.abs(ref[k][ok]) if k.startswith("focal") else 1.0
        worst = max(worst, (np.abs(main_device[k][ok] - ref[k][ok]) / scale).max())
    print(f"MODEL_SPREAD {spread:.3e} tolerance {tol:.3e} device-model worst {worst:.3e} ratio {worst / tol:.3e}")
    assert worst <= tol
    s = main_device["summary"]
    assert (s.num_pairs, s.num_too_few_correspondences) == (12, 1)
    assert s.num_estimated == int(np.count_nonzero(ref["status"] == 0))
    assert s.num_no_model == int(np.count_nonzero(ref["status"] == 2))
    assert s.total_iterations == int(ref["num_iterations"].sum())


def test_result_does_not_depend_on_the_chunking(main_device):
    for chunk in (5, 64):
        other = _run_main(chunk)
        for k in INTS + REALS + ("fundamental_matrix", "hypothesis_cost"):
            assert main_device[k].tobytes() == other[k].tobytes(), (chunk, k)
    assert _run_main(5)["summary"].num_chunks > main_device["summary"].num_chunks


def test_planted_samples():
    b = cases.planted_batch()
    ref = cases.planted_model()
    dev = lib.estimate_uncalibrated_relative_poses(b["pair_offset"], b["feature1"], b["feature2"],
                                                   np.full(3, cases.THRESHOLD), options=_options(),
                                                   samples=b["samples"], want_hypothesis_cost=True)
    _assert_equal_to_model(dev, ref)
    # two identical correspondences in the sample: rank < 8
    assert ref["results"][0].hyp[0].reason == "rank" and dev["hypothesis_cost"][0, 0] == -1
    # parallel optical axes: the model names the rejection of the focal decomposition
    assert ref["results"][1].hyp[0].reason in ("epipole_x_zero", "negative_focal_square", "nan_focal_square")
    assert ref["results"][1].hyp[0].min_margin() >= model.MARGIN and dev["hypothesis_cost"][1, 0] == -1
    # every sample degenerate
    assert dev["status"][2] == 2 and dev["num_inliers"][2] == 0 and dev["best_iteration"][2] == -1
    assert (dev["hypothesis_cost"][2] == -1).all() and dev["num_iterations"][2] == cases.MAX_ITERATIONS
    # a repeated index is an argument error
    bad = b["samples"].copy()
    bad[0, 3, 5] = bad[0, 3, 2]
    with pytest.raises(lib.EngineError) as e:
        lib.estimate_uncalibrated_relative_poses(b["pair_offset"], b["feature1"], b["feature2"],
                                                 np.full(3, cases.THRESHOLD), options=_options(), samples=bad)
    assert e.value.status == abi.ERR_INVALID_ARGUMENT


def test_mask_and_empty_batch(main_device):
    mask = np.zeros(len(cases.MAIN_COUNTS), dtype=np.uint8)
    mask[[4, 9]] = 1
    part = _run_main(pair_mask=mask)
    assert (part["status"][mask == 0] == -1).all() and part["summary"].num_pairs == 2
    po = cases.main_batch()["pair_offset"]
    for p in (4, 9):
        for k in INTS[:5] + REALS + ("fundamental_matrix",):
            assert part[k][p].tobytes() == main_device[k][p].tobytes(), (p, k)
        assert np.array_equal(part["corr_inlier"][po[p]:po[p + 1]], main_device["corr_inlier"][po[p]:po[p + 1]])
    assert np.array_equal(part["hypothesis_cost"], main_device["hypothesis_cost"][[4, 9]])  # (rows: selected pairs)
    assert part["corr_inlier"].sum() == main_device["corr_inlier"][po[4]:po[5]].sum() + main_device["corr_inlier"][po[9]:po[10]].sum()
    empty = lib.estimate_uncalibrated_relative_poses(np.zeros(1, np.int64), np.zeros((0, 2)), np.zeros((0, 2)),
                                                     np.zeros(0), options=_options())
    assert empty["status"].shape == (0,) and empty["summary"].num_pairs == 0


def test_pipeline_match_estimate_verify():
    """Descriptors at the keypoints of ONE two-view scene -> tmi_ba_match_features -> this call -> the verification BA of
    tmi_ba_verify_two_views with both focal lengths free.  The keypoints are noise-free, as the pairs of the reference's
    own focal-length test are, and the final focal lengths are held to that test's bound: kTolerance = 1e-6
    (fundamental_matrix_util_test.cc:55, :75-76).  The inlier share is held to the RANSAC test's
    (estimate_uncalibrated_relative_pose_test.cc:108-111)."""
    n, dim = 160, 32
    scene = synth.make_uncalibrated_pair_batch(1, n, 41, inlier_ratio=1.0, pixel_noise=0.0)
    rng = np.random.default_rng(7)
    pool = rng.normal(size=(n, dim))
    pool /= np.linalg.norm(pool, axis=1, keepdims=True)
    perm = rng.permutation(n)
    d1 = (pool + 0.02 * rng.normal(size=pool.shape)).astype(np.float32)
    d2 = (pool[perm] + 0.02 * rng.normal(size=pool.shape)).astype(np.float32)
    d2[: n // 8] = rng.normal(size=(n // 8, dim)).astype(np.float32) / np.sqrt(dim)  # keypoints without a partner
    m = lib.match_features(np.array([0, n, 2 * n], np.int64), np.concatenate([d1, d2]), [0], [1],
                           options=abi.match_options(device=0))
    assert m["pair_status"][0] == 0 and m["feature1"].size > 100
    i1, i2 = m["feature1"], perm[m["feature2"]]
    f1, f2 = scene["feature1"][i1], scene["feature2"][i2]
    est = lib.estimate_uncalibrated_relative_poses(np.array([0, i1.size], np.int64), f1, f2, np.array([cases.THRESHOLD]),
                                                   options=abi.two_view_ransac_options(device=0, seed=3))
    assert est["status"][0] == 0
    keep = est["corr_inlier"].astype(bool)
    assert keep.sum() > 0.7 * i1.size  # estimate_uncalibrated_relative_pose_test.cc:111
    # the TwoViewInfo as cameras: view 1 at the origin, view 2 at the estimated pose, pixels with the principal point
    pp = np.array([500.0, 400.0])
    k1 = np.zeros((1, abi.MAX_INTRINSICS))
    k2 = np.zeros((1, abi.MAX_INTRINSICS))
    k1[0, :5] = [est["focal_length1"][0], 1.0, 0.0, *pp]
    k2[0, :5] = [est["focal_length2"][0], 1.0, 0.0, *pp]
    e2 = np.concatenate([est["position"][0], est["rotation"][0]])[None]
    nk = int(keep.sum())
    batch = abi.TwoViewBatch(np.zeros((1, 6)), e2, np.zeros(1, np.int32), np.zeros(1, np.int32), k1, k2,
                             np.zeros(1, np.uint8), np.zeros(1, np.uint8), np.array([0, nk], np.int64), f1[keep] + pp,
                             f2[keep] + pp, np.zeros((nk, 4)))
    out = lib.verify_two_views(batch, device=0)
    assert out["pair_status"][0] == 0
    fl = np.array([batch.intrinsics1[0, 0], batch.intrinsics2[0, 0]])
    truth = np.array([scene["focal_length1"][0], scene["focal_length2"][0]])
    print("focal lengths after verification", fl, "truth", truth)
    assert (np.abs(fl - truth) < 1e-6).all()
