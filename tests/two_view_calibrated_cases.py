"""The inputs of tests/test_gpu_two_view_calibrated.py, in a module of their own so that
tests/test_two_view_calibrated_cpu.py can check the numpy model's decision margins on exactly them without a device.
Every model run is computed once and shared (functools.lru_cache); nobody changes the arrays."""
from __future__ import annotations

import functools
import math

import numpy as np

import two_view_calibrated_model as model
from theiasfm_amd import synth

MIN_ITERATIONS, MAX_ITERATIONS = 16, 64
MAIN_COUNTS = (4, 5, 6, 63, 64, 65, 130, 40, 77, 121, 158, 200)
MAIN_RATIOS = (1.0, 1.0, 1.0, 0.7, 0.9, 0.7, 0.9, 0.9, 0.7, 0.9, 0.7, 0.9)
MAIN_SEED, MAIN_RANSAC_SEED = 11, 5
PLANTED_SEED = 23
KW = dict(min_iterations=MIN_ITERATIONS, max_iterations=MAX_ITERATIONS)

# five_point_relative_pose_test.cc:115-190: the points, the rotation (13 degrees about z, or none), the translation,
# the noise in normalised units and the tolerance on E up to scale
FIXTURE_POINTS = ((-1.0, 3.0, 3.0), (1.0, -1.0, 2.0), (3.0, 1.0, 2.5), (-1.0, 1.0, 2.0), (2.0, 1.0, 3.0))
FIXTURE_POINTS_2 = ((-1.0, 3.0, 3.0), (1.0, -1.0, 2.0), (3.0, 1.0, 2.0), (-1.0, 1.0, 2.0), (2.0, 1.0, 3.0))
FIXTURES = dict(
    BasicMinimal=(FIXTURE_POINTS, 13.0, (1.0, 1.0, 1.0), 0.0, 1e-4),
    NoiseTestMinimal=(FIXTURE_POINTS, 13.0, (1.0, 1.0, 1.0), 1.0 / 512.0, 1e-2),
    ForwardMotionMinimal=(FIXTURE_POINTS_2, 13.0, (0.0, 0.0, 1.0), 1.0 / 512.0, 0.15),
    NoRotationMinimal=(FIXTURE_POINTS_2, 0.0, (1.0, 1.0, 1.0), 1.0 / 512.0, 0.01),
)
FIXTURE_NOISE_SEED = 67


def rotation_z(degrees):
    a = math.radians(degrees)
    return np.array([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]])


def fixture(name):
    """(x1 [5, 2], x2 [5, 2], E [3, 3] = [t]_x R of unit norm, tolerance) of one of the reference's minimal tests; the
    noise is this module's own draw (the reference's generator is not restated)."""
    pts, deg, t, noise, tol = FIXTURES[name]
    X = np.array(pts)
    R, t = rotation_z(deg), np.array(t)
    q = X @ R.T + t
    x1, x2 = X[:, :2] / X[:, 2:], q[:, :2] / q[:, 2:]
    if noise:
        rng = np.random.default_rng(FIXTURE_NOISE_SEED)
        x1 = x1 + noise * rng.normal(size=(5, 2))
        x2 = x2 + noise * rng.normal(size=(5, 2))
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    E = tx @ R
    return x1, x2, E / np.linalg.norm(E), tol


def thresholds(b):
    """(2 px)^2 / (f1 f2) per pair: RansacParameters::error_thresh in normalised units (estimate_twoview_info.cc:160-162)."""
    return 4.0 / (b["focal_length1"] * b["focal_length2"])


@functools.lru_cache(maxsize=None)
def main_batch():
    """12 pairs: the status-1 pair (4), the minimum (5), 6, the scoring wave's boundaries (63, 64, 65, 130) and five
    pairs of 40-200; 70 % inliers (the loop runs to max_iterations) or 90 % (the bound drops), half a pixel of noise at
    focal lengths of 800 to 1600."""
    return synth.make_calibrated_pair_batch(len(MAIN_COUNTS), MAIN_COUNTS, MAIN_SEED, inlier_ratio=MAIN_RATIOS,
                                            pixel_noise=0.5)


@functools.lru_cache(maxsize=None)
def main_model(path="closed", chunk=None):
    b = main_batch()
    return model.estimate(b["pair_offset"], b["feature1"], b["feature2"], thresholds(b), seed=MAIN_RANSAC_SEED,
                          path=path, chunk=chunk, **KW)


def _scene(points, deg, t, n, rng):
    X = np.concatenate([np.array(points), np.stack([rng.uniform(-2, 2, n - 5), rng.uniform(-2, 2, n - 5),
                                                    rng.uniform(2, 6, n - 5)], 1)])
    q = X @ rotation_z(deg).T + np.array(t)
    return X[:, :2] / X[:, 2:], q[:, :2] / q[:, 2:]


@functools.lru_cache(maxsize=None)
def planted_batch():
    """Four noise-free pairs with a caller's sample table:
      0  an ordinary pair of 40 whose correspondence 1 is a copy of correspondence 0; the sample of iteration 0 holds
         both (rank < 5), the other iterations are ordinary samples
      1  a pair of 6 whose correspondences 0..2 are copies of one another: every sample of five holds at least two of
         them, so every sample is degenerate (status 2)
      2  a FORWARD-MOTION pair of 40 (ForwardMotionMinimal's points, rotation and translation, then 35 more points);
         the sample of iteration 0 is the reference's five points
      3  a NO-ROTATION pair of 40 (NoRotationMinimal's), likewise"""
    rng = np.random.default_rng(PLANTED_SEED)
    b = synth.make_calibrated_pair_batch(2, (40, 6), PLANTED_SEED, inlier_ratio=1.0, pixel_noise=0.0)
    f1, f2 = b["feature1"].copy(), b["feature2"].copy()
    f1[1], f2[1] = f1[0], f2[0]
    for k in (41, 42):
        f1[k], f2[k] = f1[40], f2[40]
    fw = _scene(FIXTURE_POINTS_2, 13.0, (0.0, 0.0, 1.0), 40, rng)
    nr = _scene(FIXTURE_POINTS_2, 0.0, (1.0, 1.0, 1.0), 40, rng)
    f1 = np.concatenate([f1, fw[0], nr[0]])
    f2 = np.concatenate([f2, fw[1], nr[1]])
    po = np.array([0, 40, 46, 86, 126], np.int64)
    samples = np.zeros((4, MAX_ITERATIONS, 5), dtype=np.int32)
    for p in range(4):
        n = int(po[p + 1] - po[p])
        for i in range(MAX_ITERATIONS):
            samples[p, i] = model.sample(99, p, i, n)
    samples[0, 0] = [0, 1, 5, 9, 13]
    samples[2, 0] = samples[3, 0] = [0, 1, 2, 3, 4]
    return dict(pair_offset=po, feature1=f1, feature2=f2, samples=samples, threshold=np.full(4, 4.0e-6))


@functools.lru_cache(maxsize=None)
def planted_model():
    b = planted_batch()
    return model.estimate(b["pair_offset"], b["feature1"], b["feature2"], b["threshold"], samples=b["samples"], **KW)
