#!/usr/bin/env python
"""Throughput probe of tmi_ba_estimate_calibrated_relative_poses: P view pairs of n correspondences at a given
inlier ratio through the batched five-point RANSAC (the shape of tools/two_view_ransac_probe.py, its eight-point twin).  Reports hypotheses per second and correspondence scores per
second (over the call's kernel_seconds), kernel_seconds against the call, and which of the three per-chunk kernels
(hypothesis, score, replay) dominates.  total_scores counts correspondences x iterations; every iteration scores up to
ten models.  Appends one JSON line to profiles/two_view_calibrated_probe.jsonl.

  python tools/two_view_calibrated_probe.py [--pairs 2000] [--correspondences 300] [--inlier-ratio 0.5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from theiasfm_amd import abi, lib, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=2000)
    ap.add_argument("--correspondences", type=int, default=300)
    ap.add_argument("--inlier-ratio", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "two_view_calibrated_probe.jsonl"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    b = synth.make_calibrated_pair_batch(a.pairs, a.correspondences, 1, inlier_ratio=a.inlier_ratio, pixel_noise=0.5)
    th = 4.0 / (b["focal_length1"] * b["focal_length2"])  # (2 px)^2 in normalised units
    o = abi.two_view_ransac_options(device=0, seed=1)
    args = (b["pair_offset"], b["feature1"], b["feature2"], th)
    lib.estimate_calibrated_relative_poses(*args, options=o)  # warm-up: code object load, allocator
    runs = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        out = lib.estimate_calibrated_relative_poses(*args, options=o)
        s = out["summary"]
        runs.append((time.perf_counter() - t0, s.seconds, s.kernel_seconds, s.hypothesis_seconds, s.score_seconds,
                     s.replay_seconds))
    med = [float(np.median([r[k] for r in runs])) for k in range(6)]
    s = out["summary"]
    ok = out["status"] == 0
    phases = dict(hypothesis=med[3], score=med[4], replay=med[5])
    perr = np.degrees(np.arccos(np.clip((out["position"][ok] * b["position"][ok]).sum(1), -1.0, 1.0)))
    line = dict(what="estimate_calibrated_relative_poses", pairs=a.pairs, correspondences=a.correspondences,
                inlier_ratio=a.inlier_ratio, repeats=a.repeats, wall_seconds_median=med[0], call_seconds_median=med[1],
                kernel_seconds_median=med[2], kernel_share_of_call=med[2] / med[1] if med[1] else None,
                hypothesis_seconds_median=med[3], score_seconds_median=med[4], replay_seconds_median=med[5],
                dominant_kernel=max(phases, key=phases.get), num_chunks=int(s.num_chunks),
                total_iterations=int(s.total_iterations), total_scores=int(s.total_scores),
                hypotheses_per_second=s.total_iterations / med[2] if med[2] else None,
                scores_per_second=s.total_scores / med[2] if med[2] else None, num_estimated=int(s.num_estimated),
                num_no_model=int(s.num_no_model), median_inlier_share=float(np.median(out["num_inliers"][ok] / a.correspondences)),
                median_position_error_degrees=float(np.median(perr)) if perr.size else None)
    print(json.dumps(line), flush=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
