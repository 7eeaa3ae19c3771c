"""tmi_ba_localize_views on the device against the numpy model (tests/localization_model.py).

Shapes at which the kernels can go wrong: n in {3, 4, 30, 63, 64, 65, 257, 1000} correspondences (the scoring wavefront's
stride of 64 and its tail), V in {1, 2, 17} views, min_iterations in {1, 100}, max_iterations hit exactly, all-inlier
views (the inlier_ratio == 1 stop), a view below min_num_inliers, a view of collinear points (status 2), the five camera
models in one batch, chunk_iterations in {1, 7, 0}, the seed's samples and the caller's.

What is compared, and how:
  1. status, num_iterations, best_iteration, best_solution, num_inliers and obs_inlier: EQUAL to the model's.  The
     model evaluates the device's expressions in the device's order with correctly rounded operations only, so given
     the same correspondences its residuals are the device's bit for bit; the correspondences themselves differ by the
     rounding of pixel_to_camera (contracted on the device, libm's tan / atan2 for FOV and FISHEYE): a few ulp of O(1)
     values, i.e. below 1e-12 relative to a threshold of (4 / 900)^2 for a residual next to it.  The inputs must
     therefore have a decision margin (min |residual - thresh| / thresh over the decisive hypotheses) of at least
     RESIDUAL_DIFFERENCE_BOUND x 1000 = 1e-9, asserted on the model before anything is compared (and, without a GPU, by
     test_localization_cpu.py::test_inputs_meet_the_margin on these CASES).  The bound is an estimate from the number
     formats, not a read-back: the call has no residual output.
  2. hypothesis_cost: equal to the model's except where the model flags a residual within that margin of the threshold;
     at most 5 % of the evaluated hypotheses may be flagged.
  3. pose and confidence within max(1e-12, 100 x MODEL_SPREAD) of the model's, MODEL_SPREAD being the largest difference
     of the model's final pose between its two root paths over these inputs.
  4. identical bytes across chunk_iterations 1, 7, 0 and across two calls.
  5. with bundle_adjust_view: the extrinsics equal those of the call without it followed by tmi_ba_adjust_views on the
     status-0 mask, and the noise-free views are within 1e-4 of the truth (estimate_calibrated_absolute_pose_test.cc,
     AllInliersNoNoise)."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import localization_model as model  # noqa: E402
from theiasfm_amd import abi, lib, synth  # noqa: E402

pytestmark = pytest.mark.gpu

RESIDUAL_DIFFERENCE_BOUND = 1e-12
MARGIN = 1000 * RESIDUAL_DIFFERENCE_BOUND


def _collinear(P, c, rng):
    """Make every point camera c observes lie on one line (the points are the view's own)."""
    idx = np.nonzero(P.obs_camera == c)[0]
    t = np.linspace(-1.0, 1.0, idx.shape[0])
    P.points[P.obs_point[idx], :3] = np.outer(t, [0.3, -0.2, 0.5]) + [0.1, 0.2, -0.1]


CASES = {
    # name: (builder kwargs, option overrides, samples_given)
    "sizes": (dict(num_views=8, num_correspondences=[3, 4, 30, 63, 64, 65, 257, 1000], seed=11,
                   inlier_ratio=[1, 1, 0.7, 0.7, 0.6, 0.7, 0.5, 0.6]),
              dict(min_num_inliers=3, min_iterations=100, max_iterations=200, seed=5), False),
    "mixed17": (dict(num_views=17, num_correspondences=[80] * 14 + [10, 40, 90], seed=12,
                     inlier_ratio=[0.6] * 8 + [1.0] * 6 + [1.0, 1.0, 0.8],
                     pixel_noise=[0.5] * 8 + [0.0] * 3 + [0.5] * 6,
                     models=[0, 1, 2, 3, 4] * 3 + [0, 1]),
                dict(min_num_inliers=30, min_iterations=100, max_iterations=120, seed=77), False),
    "cap1": (dict(num_views=1, num_correspondences=65, seed=13, inlier_ratio=0.3),
             dict(min_num_inliers=3, min_iterations=1, max_iterations=5, seed=9), False),
    "given2": (dict(num_views=2, num_correspondences=[64, 257], seed=14, inlier_ratio=[0.7, 0.6]),
               dict(min_num_inliers=30, min_iterations=1, max_iterations=150, seed=0), True),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    kw, ov, given = CASES[name]
    P = synth.make_localization_batch(**kw)
    if name == "mixed17":
        # view 15's own points onto a line; give it points nobody else sees
        rng = np.random.default_rng(1)
        idx = np.nonzero(P.obs_camera == 15)[0]
        extra = np.concatenate([rng.uniform(-1, 1, (idx.shape[0], 3)), np.ones((idx.shape[0], 1))], 1)
        base = P.points.shape[0]
        P.points = np.ascontiguousarray(np.concatenate([P.points, extra]))
        P.point_constant = np.zeros(P.points.shape[0], np.uint8)
        P.obs_point[idx] = base + np.arange(idx.shape[0], dtype=np.int32)
        _collinear(P, 15, rng)
    th = P.meta["error_threshold"]
    samples = None
    if given:
        rng = np.random.default_rng(3)
        n = np.bincount(P.obs_camera, minlength=P.num_cameras)
        samples = np.stack([np.stack([rng.permutation(n[c])[:3] for _ in range(ov["max_iterations"])])
                            for c in range(P.num_cameras)]).astype(np.int32)
    mkw = dict(min_iterations=ov["min_iterations"], max_iterations=ov["max_iterations"])
    ref = model.localize(P, th, samples=samples, seed=ov["seed"], min_num_inliers=ov["min_num_inliers"], **mkw)
    alt = model.localize(P, th, samples=samples, seed=ov["seed"], min_num_inliers=ov["min_num_inliers"], roots="eigvals",
                         **mkw)
    return P, th, samples, ov, ref, alt


def _device(name, chunk, bundle_adjust_view=0):
    P, th, samples, ov, _, _ = _case(name)
    Q = P.copy()
    o = abi.localization_options(bundle_adjust_view=bundle_adjust_view, chunk_iterations=chunk, **ov)
    out = lib.localize_views(Q, th, options=o, ba_options=abi.default_options(device=0), samples=samples,
                             want_hypothesis_cost=True)
    out["extrinsics"] = Q.extrinsics
    return out


@functools.lru_cache(maxsize=None)
def _device_default(name):
    return _device(name, 0)


@pytest.mark.parametrize("name", list(CASES))
def test_decisions_equal_the_model(name):
    P, _, _, _, ref, _ = _case(name)
    assert ref["margin"] >= MARGIN
    dev = _device_default(name)
    for k in ("status", "num_correspondences", "num_iterations", "best_iteration", "best_solution", "num_inliers",
              "obs_inlier"):
        assert np.array_equal(dev[k], ref[k]), (k, dev[k], ref[k])
    if name == "mixed17":
        assert dev["status"][14] == 1 and dev["status"][15] == 2
        assert dev["num_iterations"][15] == 120
        # all-inlier views stop at min_iterations through the inlier_ratio == 1 case
        assert np.all(dev["num_iterations"][8:14] == 100)
    if name == "cap1":
        assert dev["num_iterations"][0] == 5


@pytest.mark.parametrize("name", list(CASES))
def test_hypothesis_costs(name):
    _, _, _, _, ref, _ = _case(name)
    dev = _device_default(name)
    d, m = dev["hypothesis_cost"], ref["hypothesis_cost"]
    assert d.shape == m.shape
    flagged = np.zeros(m.shape, dtype=bool)
    sel = sorted(ref["results"])
    ranks = {c: r for r, c in enumerate(np.nonzero(ref["status"] >= 0)[0])}
    for c in sel:
        for (i, k), margin in ref["results"][c].cost_margin.items():
            if margin < MARGIN:
                flagged[ranks[c], i, k] = True
    evaluated = int(np.count_nonzero(m >= 0))
    print(f"{name}: {evaluated} hypotheses, {int(flagged.sum())} flagged, {int(np.count_nonzero(d != m))} different")
    assert flagged.sum() <= 0.05 * max(evaluated, 1)
    assert np.array_equal(d[~flagged], m[~flagged])
    assert np.all(np.abs(d[flagged] - m[flagged]) <= 1)


def _pose_difference(a, b):
    return float(np.max(np.abs(a - b))) if a.size else 0.0


@pytest.mark.parametrize("name", list(CASES))
def test_pose_and_confidence(name):
    _, _, _, _, ref, alt = _case(name)
    dev = _device_default(name)
    ok = ref["status"] == 0
    assert np.array_equal(alt["status"] == 0, ok)
    spread = _pose_difference(ref["pose"][ok], alt["pose"][ok])
    tol = max(1e-12, 100 * spread)
    diff = _pose_difference(dev["extrinsics"][ok], ref["pose"][ok])
    print(f"{name}: MODEL_SPREAD {spread:.3e}, device - model {diff:.3e}, ratio {diff / max(spread, 1e-300):.3g}")
    assert diff <= tol
    assert np.max(np.abs(dev["confidence"] - ref["confidence"])) <= tol
    # views that were not localised keep their input extrinsics
    P = _case(name)[0]
    assert np.array_equal(dev["extrinsics"][~ok], P.extrinsics[~ok])


@pytest.mark.parametrize("name", list(CASES))
def test_chunks_and_repeat_give_identical_bytes(name):
    base = _device_default(name)
    for chunk in (1, 7, 0):
        other = _device(name, chunk)
        for k in ("status", "num_iterations", "best_iteration", "best_solution", "num_inliers", "obs_inlier",
                  "confidence", "hypothesis_cost", "extrinsics"):
            assert base[k].tobytes() == other[k].tobytes(), (chunk, k)


def test_bundle_adjust_view_equals_the_two_calls():
    name = "mixed17"
    P, th, samples, ov, ref, _ = _case(name)
    plain = _device_default(name)
    with_ba = _device(name, 0, bundle_adjust_view=1)
    Q = P.copy()
    Q.extrinsics[:] = plain["extrinsics"]
    mask = (plain["status"] == 0).astype(np.uint8)
    term, _, _, _, _ = lib.adjust_views(Q, abi.default_options(device=0), view_mask=mask)
    usable = (term == 0) | (term == 1)
    expect = np.where(mask.astype(bool) & ~usable, 4, plain["status"])
    assert np.array_equal(with_ba["status"], expect)
    assert with_ba["extrinsics"].tobytes() == Q.extrinsics.tobytes()
    truth = P.meta["true_extrinsics"]
    for c in (8, 9, 10):  # the noise-free all-inlier views
        assert with_ba["status"][c] == 0
        err = np.max(np.abs(with_ba["extrinsics"][c] - truth[c]))
        print(f"view {c}: |pose - truth| {err:.3e}")
        assert err < 1e-4
