"""The inputs of tests/test_gpu_homography.py, in a module of their own so that tests/test_homography_cpu.py can check
the numpy model's decision margins on exactly them without a device.  Every model run is computed once and shared
(functools.lru_cache); nobody changes the arrays.

All coordinates are NORMALISED (pixels at focal 1000 divided by 1000, principal point removed), the thresholds are in
those units squared."""
from __future__ import annotations

import functools
import math

import numpy as np

import homography_model as model

FOCAL = 1000.0
MIN_ITERATIONS, MAX_ITERATIONS = 16, 64
THRESHOLD = 4.0 / FOCAL ** 2  # 2 px, squared
MAIN_COUNTS = (3, 4, 5, 63, 64, 65, 130, 40, 77, 121, 158, 200)
MAIN_OUTLIERS = (0.0, 0.0, 0.2, 0.3, 0.1, 0.4, 0.1, 0.0, 0.3, 0.1, 0.4, 0.2)   # share of uniform outliers
MAIN_NOISE = (0.0, 0.0, 0.5, 0.5, 1.0, 0.5, 0.25, 0.0, 1.0, 0.5, 0.5, 0.75)    # pixels at focal 1000
MAIN_SEED, MAIN_RANSAC_SEED = 17, 5
PLANTED_SEED = 29
KW = dict(min_iterations=MIN_ITERATIONS, max_iterations=MAX_ITERATIONS)
MLE_PAIR = 7  # a pair of the main batch on which the two scorings pick different best iterations (the CPU test checks it)

# the reference's own scene (estimators/estimate_homography_test.cc:65-126)
REFERENCE_THRESHOLD = 16.0 / FOCAL ** 2
REFERENCE_KW = dict(failure_probability=0.001, min_iterations=100, max_iterations=1000, use_mle=True)
REFERENCE_VARIANTS = ((1.0, 0.0), (1.0, 1.0), (0.7, 0.0), (0.7, 1.0))  # (inlier ratio, noise in pixels)
REFERENCE_SEED, REFERENCE_RANSAC_SEED = 61, 7


def rotation_matrix(angle_degrees, axis):
    """Eigen's AngleAxisd(angle, axis.normalized()).toRotationMatrix()."""
    k = np.asarray(axis, dtype=np.float64)
    k = k / np.linalg.norm(k)
    t = math.radians(angle_degrees)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(t) * K + (1.0 - math.cos(t)) * (K @ K)


def plane_pair(rng, n, outlier_share, noise_pixels):
    """n correspondences of points on a tilted plane seen from two poses: (feature1, feature2, is_inlier, H) with H the
    plane's homography from image 1 to image 2."""
    R = rotation_matrix(rng.uniform(4, 12), rng.normal(size=3))
    pos = rng.uniform(-0.6, 0.6, size=3)
    normal, depth = np.array([0.3, 0.2, -1.0]), 5.0   # the plane normal . X + depth = 0, i.e. z = depth + 0.3 x + 0.2 y
    xy = rng.uniform(-2.0, 2.0, size=(n, 2))
    X = np.c_[xy, depth + 0.3 * xy[:, 0] + 0.2 * xy[:, 1]]
    Y = (X - pos) @ R.T
    f1, f2 = X[:, :2] / X[:, 2:], Y[:, :2] / Y[:, 2:]
    # Y = R (X - pos) and normal . X = -depth on the plane: Y = R (I + pos normal^T / depth) X
    H = R @ (np.eye(3) + np.outer(pos, normal) / depth)
    inlier = np.ones(n, dtype=bool)
    inlier[rng.permutation(n)[:int(round(outlier_share * n))]] = False
    k = int(np.count_nonzero(~inlier))
    f1[~inlier] = rng.uniform(-0.5, 0.5, size=(k, 2))
    f2[~inlier] = rng.uniform(-0.5, 0.5, size=(k, 2))
    f1 = f1 + rng.uniform(-1.0, 1.0, size=f1.shape) * (noise_pixels / FOCAL)
    f2 = f2 + rng.uniform(-1.0, 1.0, size=f2.shape) * (noise_pixels / FOCAL)
    return f1, f2, inlier, H


def _batch(pairs):
    counts = [p[0].shape[0] for p in pairs]
    return dict(pair_offset=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64),
                feature1=np.concatenate([p[0] for p in pairs]), feature2=np.concatenate([p[1] for p in pairs]),
                is_inlier=np.concatenate([p[2] for p in pairs]), homography=np.stack([p[3] for p in pairs]))


@functools.lru_cache(maxsize=None)
def main_batch():
    """12 pairs: the status-1 pair (3), the sample that is the whole pair (4), 5, both sides of the scoring wave's stride
    (63, 64, 65, 130) and five pairs of 40-200; 0-40 % uniform outliers, 0-1 px of noise."""
    rng = np.random.default_rng(MAIN_SEED)
    return _batch([plane_pair(rng, n, o, s) for n, o, s in zip(MAIN_COUNTS, MAIN_OUTLIERS, MAIN_NOISE)])


@functools.lru_cache(maxsize=None)
def main_model(use_mle=False, path="closed", chunk=None):
    b = main_batch()
    return model.estimate(b["pair_offset"], b["feature1"], b["feature2"], np.full(len(MAIN_COUNTS), THRESHOLD),
                          seed=MAIN_RANSAC_SEED, path=path, chunk=chunk, use_mle=use_mle, **KW)


@functools.lru_cache(maxsize=None)
def planted_batch():
    """Three noise-free pairs with a caller's sample table:
      0  a pair of 40 whose correspondences 0, 1, 2 lie on one line of the plane; the sample of iteration 0 holds the
         three and correspondence 7 (rank < 8: no model), the other iterations are ordinary samples
      1  a pair of 40 whose correspondence 1 is a copy of correspondence 0; the sample of iteration 0 holds both
      2  a pair of 6 whose correspondences 0..3 are copies of one another: every sample of four holds at least two of
         them, so every sample is degenerate"""
    rng = np.random.default_rng(PLANTED_SEED)
    pairs = [plane_pair(rng, n, 0.0, 0.0) for n in (40, 40, 6)]
    f1, f2 = pairs[0][0], pairs[0][1]
    # three points of the image-1 line y = 0.125 x + 0.0625 (exact binary fractions) and their images under the pair's H
    H = pairs[0][3]
    for k, x in enumerate((-0.25, 0.0, 0.375)):
        f1[k] = (x, 0.125 * x + 0.0625)
        q = H @ np.array([f1[k, 0], f1[k, 1], 1.0])
        f2[k] = q[:2] / q[2]
    pairs[1][0][1], pairs[1][1][1] = pairs[1][0][0], pairs[1][1][0]
    for k in range(1, 4):
        pairs[2][0][k], pairs[2][1][k] = pairs[2][0][0], pairs[2][1][0]
    b = _batch(pairs)
    po = b["pair_offset"]
    samples = np.zeros((3, MAX_ITERATIONS, 4), dtype=np.int32)
    for p in range(3):
        n = int(po[p + 1] - po[p])
        for i in range(MAX_ITERATIONS):
            samples[p, i] = model.sample(99, p, i, n)
    samples[0, 0] = [0, 1, 2, 7]
    samples[1, 0] = [0, 1, 5, 9]
    b["samples"] = samples
    return b


@functools.lru_cache(maxsize=None)
def planted_model(use_mle=False):
    b = planted_batch()
    return model.estimate(b["pair_offset"], b["feature1"], b["feature2"], np.full(3, THRESHOLD), samples=b["samples"],
                          use_mle=use_mle, **KW)


@functools.lru_cache(maxsize=None)
def reference_batch():
    """estimate_homography_test.cc:65-126: the 9x9 lattice at depth 5, three rotations times two positions, in the four
    variants of REFERENCE_VARIANTS: 24 pairs of 81, variant-major."""
    rng = np.random.default_rng(REFERENCE_SEED)
    X = np.array([[i, j, 5.0] for i in range(-4, 5) for j in range(-4, 5)], dtype=np.float64)
    rotations = (np.eye(3), rotation_matrix(12.0, (0, 1, 0)), rotation_matrix(-9.0, (1.0, 0.2, -0.8)))
    positions = (np.array([-1.3, 0.0, 0.0]), np.array([0.0, 0.0, 0.5]))
    pairs = []
    for ratio, noise in REFERENCE_VARIANTS:
        for R in rotations:
            for pos in positions:
                t = -R @ pos
                t = t / np.linalg.norm(t)
                Y = X @ R.T + t
                f1, f2 = X[:, :2] / X[:, 2:], Y[:, :2] / Y[:, 2:]
                inlier = np.arange(81) < ratio * 81
                k = int(np.count_nonzero(~inlier))
                f1[~inlier] = rng.uniform(-1.0, 1.0, size=(k, 2))
                f2[~inlier] = rng.uniform(-1.0, 1.0, size=(k, 2))
                if noise:
                    f1 = f1 + rng.normal(size=f1.shape) * (noise / FOCAL)
                    f2 = f2 + rng.normal(size=f2.shape) * (noise / FOCAL)
                pairs.append((f1, f2, inlier, np.eye(3)))
    return _batch(pairs)


@functools.lru_cache(maxsize=None)
def reference_model():
    b = reference_batch()
    return model.estimate(b["pair_offset"], b["feature1"], b["feature2"], np.full(24, REFERENCE_THRESHOLD),
                          seed=REFERENCE_RANSAC_SEED, **REFERENCE_KW)
