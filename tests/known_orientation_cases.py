"""The inputs of tests/test_gpu_known_orientation.py, in a module of their own so that
tests/test_known_orientation_cpu.py can check the numpy model's decision margins on exactly them without a device.
Every model run is computed once and shared (functools.lru_cache); nobody changes the arrays.

All features are NORMALISED (pixels at focal 1000 divided by 1000, principal point removed) and NOT rotated: each item
carries its view's angle-axis (the relative items two).  The thresholds are in those units squared.  `kind` is
"absolute" (tmi_ba_estimate_positions_known_orientation) or "relative"
(tmi_ba_estimate_relative_positions_known_orientation)."""
from __future__ import annotations

import functools
import math

import numpy as np

import known_orientation_model as model
from track_estimator_model import angle_axis_to_rotation_matrix

KINDS = ("absolute", "relative")
FOCAL = 1000.0
MIN_ITERATIONS, MAX_ITERATIONS = 16, 64
THRESHOLD = 4.0 / FOCAL ** 2  # 2 px, squared
# item:         0    1    2     3     4     5     6      7         8           9
#               one sample     the MLE sum's lane stride   status 1  masked  degenerate  40 % gross outliers
MAIN_COUNTS = (2, 3, 63, 64, 65, 130, 1, 20, 12, 100)
MAIN_OUTLIERS = (0.0, 0.0, 0.2, 0.1, 0.3, 0.1, 0.0, 0.0, 0.0, 0.4)
MAIN_NOISE = (0.0, 0.5, 0.5, 1.0, 0.5, 0.25, 0.0, 0.5, 0.0, 0.5)  # pixels at focal 1000, uniform
STATUS1_ITEM, MASKED_ITEM, DEGENERATE_ITEM, OUTLIER_ITEM = 6, 7, 8, 9
MAIN_MASK = np.array([1, 1, 1, 1, 1, 1, 1, 0, 1, 1], dtype=np.uint8)
MAIN_SEED, MAIN_RANSAC_SEED = {"absolute": 23, "relative": 31}, 5
PLANTED_SEED = 41
KW = dict(min_iterations=MIN_ITERATIONS, max_iterations=MAX_ITERATIONS)
# an item of the main batch on which the two scorings pick different best iterations (the CPU test checks it)
MLE_ITEM = {"absolute": 3, "relative": 2}

# the reference's own scenes (estimate_absolute_pose_with_known_orientation_test.cc:61-240,
# estimate_relative_pose_with_known_orientation_test.cc:61-237): 100 points, 4 px threshold at focal 1000
REFERENCE_POINTS = 100
REFERENCE_THRESHOLD = 16.0 / FOCAL ** 2
REFERENCE_KW = dict(failure_probability=0.001, min_iterations=100, max_iterations=1000, use_mle=True)
# (inlier ratio, noise in pixels, pose tolerance, uses the random rotation): :127-155, :157-186, :188-213, :215-240
REFERENCE_VARIANTS = ((1.0, 0.0, 1e-4, False), (1.0, 1.0, 1e-2, False), (0.7, 0.0, 1e-2, True), (0.7, 1.0, 1e-2, True))
REFERENCE_SEED, REFERENCE_RANSAC_SEED = 66, 7


def angle_axis(angle_degrees, axis):
    k = np.asarray(axis, dtype=np.float64)
    return math.radians(angle_degrees) * k / np.linalg.norm(k)


def _project(R, X):
    Y = X @ R.T
    return Y[:, :2] / Y[:, 2:]


def _noise_and_outliers(rng, features, outlier_share, noise_pixels):
    n = features[0].shape[0]
    inlier = np.ones(n, dtype=bool)
    inlier[rng.permutation(n)[:int(round(outlier_share * n))]] = False
    k = int(np.count_nonzero(~inlier))
    for f in features:
        f[~inlier] = rng.uniform(-1.0, 1.0, size=(k, 2))
        f += rng.uniform(-1.0, 1.0, size=f.shape) * (noise_pixels / FOCAL)
    return inlier


def make_item(kind, rng, n, outlier_share, noise_pixels, orientations=None, position=None):
    """One view (absolute) or view pair (relative) of n correspondences: a dict with features [list of [n, 2]],
    orientations [list of [3]], world_point [n, 3], position [3] (the truth; relative: the baseline c2 - c1)."""
    X = np.c_[rng.uniform(-2.0, 2.0, size=(n, 2)), rng.uniform(6.0, 10.0, size=n)]
    pos = rng.uniform(-1.0, 1.0, size=3) if position is None else np.asarray(position, dtype=np.float64)
    count = 1 if kind == "absolute" else 2
    aas = [angle_axis(rng.uniform(3.0, 12.0), rng.normal(size=3)) for _ in range(count)] if orientations is None \
        else [np.asarray(a, dtype=np.float64) for a in orientations]
    Rs = [angle_axis_to_rotation_matrix(a) for a in aas]
    if kind == "absolute":
        features = [_project(Rs[0], X - pos)]
    else:
        features = [_project(Rs[0], X), _project(Rs[1], X - pos)]
    inlier = _noise_and_outliers(rng, features, outlier_share, noise_pixels)
    return dict(features=features, orientations=aas, world_point=X, position=pos, is_inlier=inlier)


def make_degenerate(kind, rng, n):
    """Every sample rank deficient, exactly.  absolute: n world points on ONE ray through the camera centre, so all
    features are the same two doubles (q == 0).  relative: no baseline and one rotation for both views, feature2 ==
    feature1, so every epipolar row is (0, 0, 0)."""
    it = make_item(kind, rng, n, 0.0, 0.0)
    if kind == "absolute":
        R = angle_axis_to_rotation_matrix(it["orientations"][0])
        f = np.array([0.125, -0.0625])
        it["features"][0][:] = f
        it["world_point"] = it["position"] + np.outer(rng.uniform(4.0, 9.0, size=n), R.T @ np.array([f[0], f[1], 1.0]))
    else:
        it["orientations"][1] = it["orientations"][0].copy()
        it["features"][1] = it["features"][0].copy()
        it["position"] = np.zeros(3)
    return it


def _batch(kind, items):
    counts = [it["features"][0].shape[0] for it in items]
    k = len(items[0]["features"])
    return dict(kind=kind, item_offset=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64),
                features=[np.concatenate([it["features"][j] for it in items]) for j in range(k)],
                orientations=[np.stack([it["orientations"][j] for it in items]) for j in range(k)],
                world_point=np.concatenate([it["world_point"] for it in items]) if kind == "absolute" else None,
                position=np.stack([it["position"] for it in items]),
                is_inlier=np.concatenate([it["is_inlier"] for it in items]))


@functools.lru_cache(maxsize=None)
def main_batch(kind):
    rng = np.random.default_rng(MAIN_SEED[kind])
    items = []
    for p, (n, o, s) in enumerate(zip(MAIN_COUNTS, MAIN_OUTLIERS, MAIN_NOISE)):
        items.append(make_degenerate(kind, rng, n) if p == DEGENERATE_ITEM else make_item(kind, rng, n, o, s))
    return _batch(kind, items)


def run_model(b, thresholds, rotated=None, **kw):
    return model.estimate(b["kind"], b["item_offset"], b["features"], b["orientations"], thresholds,
                          world_point=b["world_point"], rotated=rotated, **kw)


@functools.lru_cache(maxsize=None)
def main_model(kind, use_mle=False, path="closed", chunk=None):
    """The model on its OWN rotation (math.sin / math.cos); the GPU test runs it again on the device's."""
    return run_model(main_batch(kind), np.full(len(MAIN_COUNTS), THRESHOLD), item_mask=MAIN_MASK,
                     seed=MAIN_RANSAC_SEED, path=path, chunk=chunk, use_mle=use_mle, **KW)


@functools.lru_cache(maxsize=None)
def planted_batch(kind):
    """Three noise-free items with a caller's sample table:
      0  30 correspondences of which 1 is a copy of 0; the sample of iteration 0 holds the two (rank deficient: no
         model), the other iterations are ordinary samples
      1  30 ordinary correspondences, every sample drawn from another seed than the call's
      2  the degenerate item: every sample without a model"""
    rng = np.random.default_rng(PLANTED_SEED)
    items = [make_item(kind, rng, 30, 0.0, 0.0), make_item(kind, rng, 30, 0.0, 0.0), make_degenerate(kind, rng, 5)]
    for f in items[0]["features"]:
        f[1] = f[0]
    items[0]["world_point"][1] = items[0]["world_point"][0]
    b = _batch(kind, items)
    po = b["item_offset"]
    samples = np.zeros((3, MAX_ITERATIONS, 2), dtype=np.int32)
    for p in range(3):
        for i in range(MAX_ITERATIONS):
            samples[p, i] = model.sample(99, p, i, int(po[p + 1] - po[p]))
    samples[0, 0] = [0, 1]
    b["samples"] = samples
    return b


@functools.lru_cache(maxsize=None)
def planted_model(kind, use_mle=False):
    b = planted_batch(kind)
    return run_model(b, np.full(3, THRESHOLD), samples=b["samples"], use_mle=use_mle, **KW)


@functools.lru_cache(maxsize=None)
def reference_batch(kind):
    """The scenes of the reference's four estimator tests: 100 points in [-2, 2]^2 x [6, 10]; variants 0 and 1 with the
    three fixed rotations times the positions (-1.3, 0, 0), (0, 0, 0.5), variants 2 and 3 with the identity and a random
    10-degree rotation times (1, 0, 0), (0, 1, 0): 20 items, variant-major.  The first i < ratio * 100 correspondences
    are inliers, the others uniform in [-1, 1]^2; the noise is uniform.  In the relative scenes the reference never uses
    its rotation (its features are generated in one frame); here it is the SECOND view's, the first view's the identity,
    so that the scene is the reference's once rotated back."""
    rng = np.random.default_rng(REFERENCE_SEED)
    fixed = (np.zeros(3), angle_axis(12.0, (0, 1, 0)), angle_axis(-9.0, (1.0, 0.2, -0.8)))
    items, tolerance = [], []
    for ratio, noise, tol, random_rotation in REFERENCE_VARIANTS:
        if random_rotation:
            rotations = (np.zeros(3), angle_axis(10.0, rng.uniform(-1.0, 1.0, size=3)))
            positions = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0))
        else:
            rotations, positions = fixed, ((-1.3, 0.0, 0.0), (0.0, 0.0, 0.5))
        for aa in rotations:
            for pos in positions:
                it = make_item(kind, rng, REFERENCE_POINTS, 0.0, 0.0, position=pos,
                               orientations=[aa] if kind == "absolute" else [np.zeros(3), aa])
                out = np.arange(REFERENCE_POINTS) >= ratio * REFERENCE_POINTS
                for f in it["features"]:
                    f[out] = rng.uniform(-1.0, 1.0, size=(int(out.sum()), 2))
                    if noise:
                        f += rng.uniform(-1.0, 1.0, size=f.shape) * (noise / FOCAL)
                it["is_inlier"] = ~out
                items.append(it)
                tolerance.append(tol)
    b = _batch(kind, items)
    b["tolerance"] = np.array(tolerance)
    return b


@functools.lru_cache(maxsize=None)
def reference_model(kind):
    b = reference_batch(kind)
    return run_model(b, np.full(len(b["tolerance"]), REFERENCE_THRESHOLD), seed=REFERENCE_RANSAC_SEED, **REFERENCE_KW)


# position_from_two_rays_test.cc:108-134 and relative_pose_from_two_points_with_known_rotation_test.cc:100-126
SOLVER_POINTS = (
    (-1.62, -2.99, 6.12, 4.42, -1.53, 9.83), (1.45, -0.59, 5.29, 1.89, -1.10, 8.22), (-0.21, 2.38, 5.63, 0.61, -0.97, 7.49),
    (0.48, 0.70, 8.94, 1.65, -2.56, 8.63), (2.44, -0.20, 7.78, 2.84, -2.58, 7.35), (-1.35, -2.84, 7.33, -0.42, 1.54, 8.86),
    (2.56, 1.72, 7.86, 1.75, -1.39, 5.73), (2.08, -3.91, 8.37, -0.91, 1.36, 9.16), (2.84, 1.54, 8.74, -1.01, 3.02, 8.18),
    (-3.73, -0.62, 7.81, -2.98, -1.88, 6.23), (2.39, -0.19, 6.47, -0.63, -1.05, 7.11), (-1.76, -0.55, 5.18, -3.19, 3.27, 8.18),
    (0.31, -2.77, 7.54, 0.54, -3.77, 9.77))
SOLVER_BASIC_POINTS = (5.0, 20.0, 23.0, -6.0, 16.0, 33.0)
SOLVER_BASIC_POSITION = (-3.0, 1.5, 11.0)
SOLVER_POSITIONS = {  # (ManyPointsTest, DifferentAxesTest): they differ in the fifth entry
    "absolute": (((1.0, 1.0, 1.0), (3.0, 2.0, 13.0), (4.0, 5.0, 11.0), (1.0, 2.0, 15.0), (3.0, 1.5, 91.0), (1.0, 7.0, 11.0),
                  (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)), (3.0, 1.5, 21.0)),
    "relative": (((1.0, 1.0, 1.0), (3.0, 2.0, 13.0), (4.0, 5.0, 11.0), (1.0, 2.0, 15.0), (3.0, 1.5, 91.0), (1.0, 7.0, 11.0),
                  (1.0, 0.0, 0.0), (0.0, 0.0, 1.0)), (3.0, 1.5, 21.0)),
}
SOLVER_TOLERANCE = 1e-4  # kTolerance, :67 of both files


def solver_cases(kind):
    """(two points [6], position [3]) of BasicTest, DifferentAxesTest and ManyPointsTest."""
    many, fifth = SOLVER_POSITIONS[kind]
    cases = [(SOLVER_BASIC_POINTS, SOLVER_BASIC_POSITION)]
    cases += [(SOLVER_BASIC_POINTS, fifth if k == 4 else pos) for k, pos in enumerate(many)]
    cases += [(pts, pos) for pts in SOLVER_POINTS for pos in many]
    return cases
