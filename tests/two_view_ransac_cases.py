"""The inputs of tests/test_gpu_two_view_ransac.py, in a module of their own so that tests/test_two_view_ransac_cpu.py
can check the numpy model's decision margins on exactly them without a device.  Every model run is computed once and
shared (functools.lru_cache); nobody changes the arrays."""
from __future__ import annotations

import functools

import numpy as np

import two_view_ransac_model as model
from theiasfm_amd import synth

MIN_ITERATIONS, MAX_ITERATIONS = 16, 64
THRESHOLD = 4.0  # pixels^2: 2 px in each image
MAIN_COUNTS = (7, 8, 9, 63, 64, 65, 130, 40, 77, 121, 158, 200)
MAIN_RATIOS = (1.0, 0.75, 0.8, 0.7, 0.9, 0.7, 0.9, 0.9, 0.7, 0.9, 0.7, 0.9)
MAIN_SEED, MAIN_RANSAC_SEED = 11, 5
PLANTED_SEED = 23
KW = dict(min_iterations=MIN_ITERATIONS, max_iterations=MAX_ITERATIONS)


@functools.lru_cache(maxsize=None)
def main_batch():
    """12 pairs: the status-1 pair (7), the minimum (8), n not a multiple of 8, the scoring wave's boundaries (63, 64,
    65, 130) and five pairs of 40-200; 70 % inliers (the loop runs to max_iterations) or 90 % (the bound drops), half a
    pixel of noise."""
    return synth.make_uncalibrated_pair_batch(len(MAIN_COUNTS), MAIN_COUNTS, MAIN_SEED, inlier_ratio=MAIN_RATIOS,
                                              pixel_noise=0.5)


@functools.lru_cache(maxsize=None)
def main_model(path="closed", chunk=None):
    b = main_batch()
    return model.estimate(b["pair_offset"], b["feature1"], b["feature2"], np.full(len(MAIN_COUNTS), THRESHOLD),
                          seed=MAIN_RANSAC_SEED, path=path, chunk=chunk, **KW)


@functools.lru_cache(maxsize=None)
def planted_batch():
    """Three pairs with a caller's sample table:
      0  an ordinary pair of 40 whose correspondence 1 is a copy of correspondence 0; the sample of iteration 0 holds
         both (rank < 8), the other iterations are ordinary samples
      1  a pair of 40 whose views share PARALLEL optical axes (view 2 is not turned): the focal lengths are not
         recoverable and the decomposition of iteration 0's all-inlier sample is rejected
      2  a pair of 10 whose correspondences 0..4 are copies of one another: every sample of eight holds at least three
         of them, so every sample is degenerate"""
    b = synth.make_uncalibrated_pair_batch(3, (40, 40, 10), PLANTED_SEED, inlier_ratio=1.0, pixel_noise=0.0,
                                           parallel_axes=(1,))
    f1, f2 = b["feature1"].copy(), b["feature2"].copy()
    po = b["pair_offset"]
    f1[po[0] + 1], f2[po[0] + 1] = f1[po[0]], f2[po[0]]
    for k in range(1, 5):
        f1[po[2] + k], f2[po[2] + k] = f1[po[2]], f2[po[2]]
    samples = np.zeros((3, MAX_ITERATIONS, 8), dtype=np.int32)
    for p in range(3):
        n = int(po[p + 1] - po[p])
        for i in range(MAX_ITERATIONS):
            samples[p, i] = model.sample(99, p, i, n)
    samples[0, 0] = [0, 1, 5, 9, 13, 17, 21, 25]
    samples[1, 0] = [2, 7, 11, 16, 22, 27, 33, 38]
    return dict(pair_offset=po, feature1=f1, feature2=f2, samples=samples)


@functools.lru_cache(maxsize=None)
def planted_model():
    b = planted_batch()
    return model.estimate(b["pair_offset"], b["feature1"], b["feature2"], np.full(3, THRESHOLD), samples=b["samples"],
                          **KW)
