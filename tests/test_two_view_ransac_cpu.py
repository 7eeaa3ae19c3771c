"""The numpy model of tmi_ba_estimate_uncalibrated_relative_poses (tests/two_view_ransac_model.py) on its own, and the
call's argument errors through the C ABI (which come before the device is looked for): no GPU needed.

Tolerances on noise-free pairs are the reference's own tests':
  F        eight_point_fundamental_matrix_test.cc:156-157 -- kNoise 0, kMaxReprojectionError = 1e-12, a SQUARED
           reprojection error in normalised image coordinates (:113-119); held here as the squared Sampson distance
           (the first-order reprojection error) of every true correspondence under the estimated F, in pixels^2 divided
           by f1 f2
  focal    fundamental_matrix_util_test.cc:55, :75-76 -- kTolerance = 1e-6, absolute
  pose     estimate_uncalibrated_relative_pose_test.cc:108-111 checks only that the inlier ratio exceeds 0.7 x the true
           one; that is asserted, and the rotation and the unit position are held to the focal test's 1e-6 as well"""
import math
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


@pytest.fixture(scope="module")
def noise_free():
    b = synth.make_uncalibrated_pair_batch(4, 60, 3, inlier_ratio=1.0, pixel_noise=0.0)
    runs = {path: model.estimate(b["pair_offset"], b["feature1"], b["feature2"], np.full(4, cases.THRESHOLD), seed=1,
                                 path=path, **cases.KW) for path in ("closed", "numpy")}
    return b, runs


def test_noise_free_pairs(noise_free):
    b, runs = noise_free
    for path, o in runs.items():
        assert (o["status"] == 0).all()
        assert (o["num_inliers"] > 0.7 * 1.0 * o["num_correspondences"]).all()  # ..._relative_pose_test.cc:111
        for k in ("focal_length1", "focal_length2"):
            assert np.abs(o[k] - b[k]).max() < 1e-6, (path, k)  # fundamental_matrix_util_test.cc:55
        assert np.abs(o["rotation"] - b["rotation"]).max() < 1e-6 and np.abs(o["position"] - b["position"]).max() < 1e-6
        Fm = o["fundamental_matrix"].reshape(-1, 3, 3).transpose(0, 2, 1)
        for p in range(4):
            a, e = int(b["pair_offset"][p]), int(b["pair_offset"][p + 1])
            x1 = np.c_[b["feature1"][a:e], np.ones(e - a)]
            x2 = np.c_[b["feature2"][a:e], np.ones(e - a)]
            l, g = x1 @ Fm[p].T, x2 @ Fm[p]
            sampson = np.einsum("ij,ij->i", x2, l) ** 2 / (l[:, 0] ** 2 + l[:, 1] ** 2 + g[:, 0] ** 2 + g[:, 1] ** 2)
            assert (sampson / (b["focal_length1"][p] * b["focal_length2"][p])).max() < 1e-12  # eight_point_..._test.cc:157
            # up to scale and sign: the same matrix as the truth
            assert np.abs(model.unit_f(o["fundamental_matrix"][p]) - model.unit_f(b["fundamental_matrix"][p].T.reshape(9))).max() < 1e-6


def test_the_two_model_paths_agree(noise_free):
    """MODEL_SPREAD per input (DESIGN 8.10 records the values): both paths pick the same best iteration with the same
    integers, and differ in the real outputs by no more than a conditioning-sized multiple of the unit roundoff."""
    _, runs = noise_free
    spreads = {"noise_free": model.model_spread(runs["closed"], runs["numpy"]),
               "main": model.model_spread(cases.main_model(), cases.main_model("numpy"))}
    print("MODEL_SPREAD", spreads)
    for name, (a, c) in {"noise_free": (runs["closed"], runs["numpy"]),
                         "main": (cases.main_model(), cases.main_model("numpy"))}.items():
        same = a["best_iteration"] == c["best_iteration"]
        # where the best iteration differs the two paths found equal costs through differently ordered candidates
        assert np.array_equal(a["num_inliers"][same], c["num_inliers"][same]), name
        assert spreads[name] < 1e-9, name  # 1e-9: the margin below which a decision counts as open


def test_focal_lengths_do_not_depend_on_the_sign_of_the_epipoles():
    b = cases.main_batch()
    a, e = int(b["pair_offset"][6]), int(b["pair_offset"][7])
    idx = np.flatnonzero(b["is_inlier"][a:e])[:8] + a
    h = model.hypothesis(*[[float(v) for v in b[k][idx, c]] for k, c in (("feature1", 0), ("feature1", 1),
                                                                            ("feature2", 0), ("feature2", 1))])
    assert h.ok
    base = model.focal_lengths(h.F)
    assert base[2] == "" and (base[0], base[1]) == (h.f1, h.f2)
    for flips in ((True, False), (False, True), (True, True)):
        f1, f2, reason, _ = model.focal_lengths(h.F, *flips)
        assert reason == "" and abs(f1 - h.f1) <= 1e-12 * h.f1 and abs(f2 - h.f2) <= 1e-12 * h.f2


@pytest.mark.parametrize("name", ["main", "planted"])
def test_margins_on_the_gpu_tests_inputs(name):
    """What tests/test_gpu_two_view_ransac.py relies on: at most 2 % of the replayed hypotheses have a decision margin
    below 1e-9, and none of those is the best model of its pair or changes its pair's bound.  1e-9 is the margin of
    the localisation call's test with the same caveat: it is a RELATIVE distance of a computed quantity
    to its threshold, far above the few ulps by which device and model could differ only if they evaluated different
    expressions -- they evaluate the same ones, so the margin guards against a compiler that reassociates, not
    against expected noise.  The vote's gap is an integer and flags nothing by itself (two_view_ransac_model.py);
    where a best model's gap is 0 the two PATHS may differ, which MODEL_SPREAD then shows."""
    o = cases.main_model() if name == "main" else cases.planted_model()
    replayed = sum(len(r.hyp) for r in o["results"].values())
    flagged = sum(len(r.flagged) for r in o["results"].values())
    print(name, "replayed", replayed, "flagged", flagged)
    assert replayed > 0 and flagged <= 0.02 * replayed
    for p, r in o["results"].items():
        assert r.best_iteration not in r.flagged, p
        assert not (r.flagged & r.bound_changers), p
    if name == "main":
        assert any(r.bound_changers for r in o["results"].values())  # the bound does drop somewhere


def test_sampler_properties():
    for n in (8, 9, 13, 64, 200):
        seen = set()
        for i in range(200):
            s = model.sample(7, 3, i, n)
            assert len(set(s)) == 8 and min(s) >= 0 and max(s) < n
            seen.update(s)
        assert seen == set(range(n))
    assert model.sample(7, 3, 0, 50) != model.sample(7, 4, 0, 50) and model.sample(7, 3, 0, 50) != model.sample(8, 3, 0, 50)
    assert model.sample(7, 3, 5, 50) == model.sample(7, 3, 5, 50)
    counts = np.zeros(20)
    for i in range(4000):
        counts[list(model.sample(1, 0, i, 20))] += 1
    assert np.abs(counts / 4000 - 0.4).max() < 0.04  # every index in 8 of 20 samples, four standard deviations


def _reference_loop(costs, n, failure_probability, min_iterations, max_iterations):
    """sample_consensus_estimator.h:276-330 over precomputed costs (None: EstimateModel returned false)."""
    log_fp = math.log(failure_probability)
    best_cost, best_it, bound, it = float("inf"), -1, max_iterations, 0
    while it < bound:
        c = costs[it]
        it += 1
        if c is None:
            continue
        if c < best_cost:
            best_cost, best_it = c, it - 1
            ratio = (n - c) / n
            if ratio < 8 / n:
                continue
            bound = min(model.compute_max_iterations(ratio, log_fp, min_iterations, max_iterations), bound)
    return it, best_it


def test_replay_against_the_reference_loop():
    for o in (cases.main_model(), cases.main_model("closed", 5), cases.planted_model()):
        for p, r in o["results"].items():
            costs = [r.hyp[i].cost if i in r.hyp and r.hyp[i].ok else None for i in range(cases.MAX_ITERATIONS)]
            assert _reference_loop(costs, r.n, 0.01, cases.MIN_ITERATIONS, cases.MAX_ITERATIONS) == \
                (r.num_iterations, r.best_iteration), p
    a, c = cases.main_model(), cases.main_model("closed", 5)
    for k in ("status", "num_inliers", "num_iterations", "best_iteration", "hypothesis_cost", "corr_inlier"):
        assert np.array_equal(a[k], c[k]), k
    assert model.compute_max_iterations(1.0, math.log(0.01), 16, 64) == 16
    assert model.compute_max_iterations(0.5, math.log(0.01), 10, 5000) == 1176  # log(0.01) / log(1 - 2^-8)


def test_argument_errors():
    """Returned before the device is looked for, so they need none."""
    b = cases.planted_batch()
    po, f1, f2, sm = b["pair_offset"], b["feature1"], b["feature2"], b["samples"]
    th = np.full(3, cases.THRESHOLD)

    def status(**kw):
        args = dict(pair_offset=po, feature1=f1, feature2=f2, pair_error_threshold=th,
                    options=abi.two_view_ransac_options(**cases.KW))
        args.update(kw)
        with pytest.raises(lib.EngineError) as e:
            lib.estimate_uncalibrated_relative_poses(**args)
        return e.value.status

    bad = sm.copy()
    bad[1, 7, 0] = bad[1, 7, 4]
    assert status(samples=bad) == abi.ERR_INVALID_ARGUMENT
    bad = sm.copy()
    bad[2, 0, 3] = 10
    assert status(samples=bad) == abi.ERR_INVALID_ARGUMENT
    assert status(pair_error_threshold=np.array([4.0, 0.0, 4.0])) == abi.ERR_INVALID_ARGUMENT
    assert status(pair_offset=np.array([0, 40, 30, 90])) == abi.ERR_INVALID_ARGUMENT
    assert status(pair_offset=np.array([1, 40, 80, 90])) == abi.ERR_INVALID_ARGUMENT
    for kw in (dict(failure_probability=0.0), dict(failure_probability=1.0), dict(min_inlier_ratio=1.5),
               dict(min_iterations=65, max_iterations=64), dict(max_iterations=(1 << 20) + 1),
               dict(chunk_iterations=-1)):
        assert status(options=abi.two_view_ransac_options(**kw)) == abi.ERR_INVALID_ARGUMENT, kw
    # a bad sample of a pair that is NOT attempted (masked out) is not looked at: the call gets as far as the device
    bad = sm.copy()
    bad[1, 7, 0] = bad[1, 7, 4]
    try:
        lib.estimate_uncalibrated_relative_poses(po, f1, f2, th, options=abi.two_view_ransac_options(**cases.KW),
                                                 pair_mask=[1, 0, 1], samples=bad)
    except lib.EngineError as e:
        assert e.status != abi.ERR_INVALID_ARGUMENT
    o = abi.two_view_ransac_options()
    L = lib.load()
    c = abi.CTwoViewRansacOptions()
    L.tmi_ba_two_view_ransac_options_init(c)
    for name, _ in abi.CTwoViewRansacOptions._fields_:
        assert getattr(o, name) == getattr(c, name), name
    assert (c.min_iterations, c.max_iterations, c.failure_probability) == (10, 1000, 0.01)
