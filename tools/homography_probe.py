#!/usr/bin/env python
"""Throughput probe of tmi_ba_estimate_homographies: P view pairs of n correspondences of a plane at a given inlier
ratio through the batched four-point RANSAC, under both scorings (inlier count, MLESAC).  Reports hypotheses per second
and correspondence scores per second (over the call's kernel_seconds), kernel_seconds against the call, and the
hypothesis / score / replay split from the summary.  The eight-point call (tmi_ba_estimate_uncalibrated_relative_poses)
runs on the SAME batch in the same process, so that the two figures come from one box and one job.  Appends one JSON
line per call to profiles/homography_probe.jsonl.

  python tools/homography_probe.py [--pairs 20000] [--correspondences 300] [--inlier-ratio 0.5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from theiasfm_amd import abi, lib  # noqa: E402

FOCAL = 1000.0


def make_plane_batch(pairs, n, inlier_ratio, pixel_noise, seed):
    """`pairs` view pairs of n correspondences each, in centred pixels at focal 1000: points of a tilted plane seen from
    two poses (a turn of up to 0.2 rad about y, a shift), the share 1 - inlier_ratio replaced by uniform pixels."""
    rng = np.random.default_rng(seed)
    ang = rng.uniform(-0.2, 0.2, size=(pairs, 1))
    pos = rng.uniform(-0.5, 0.5, size=(pairs, 1, 3))
    x = rng.uniform(-2.0, 2.0, size=(pairs, n))
    y = rng.uniform(-2.0, 2.0, size=(pairs, n))
    z = 5.0 + 0.3 * x + 0.2 * y
    d = np.stack([x, y, z], axis=2) - pos
    c, s = np.cos(ang), np.sin(ang)
    q = np.stack([c * d[..., 0] + s * d[..., 2], d[..., 1], -s * d[..., 0] + c * d[..., 2]], axis=2)
    f1 = FOCAL * np.stack([x / z, y / z], axis=2)
    f2 = FOCAL * q[..., :2] / q[..., 2:]
    out = rng.uniform(size=(pairs, n)) >= inlier_ratio
    f1[out] = rng.uniform(-500.0, 500.0, size=(int(out.sum()), 2))
    f2[out] = rng.uniform(-500.0, 500.0, size=(int(out.sum()), 2))
    f1 += rng.uniform(-pixel_noise, pixel_noise, size=f1.shape)
    f2 += rng.uniform(-pixel_noise, pixel_noise, size=f2.shape)
    po = np.arange(pairs + 1, dtype=np.int64) * n
    return po, f1.reshape(-1, 2), f2.reshape(-1, 2)


def measure(call, repeats):
    call()  # warm-up: code object load, allocator
    runs = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = call()
        s = out["summary"]
        runs.append((time.perf_counter() - t0, s.seconds, s.kernel_seconds, s.hypothesis_seconds, s.score_seconds,
                     s.replay_seconds))
    return out, [float(np.median([r[k] for r in runs])) for k in range(6)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=20000)
    ap.add_argument("--correspondences", type=int, default=300)
    ap.add_argument("--inlier-ratio", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "homography_probe.jsonl"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    po, f1, f2 = make_plane_batch(a.pairs, a.correspondences, a.inlier_ratio, 0.5, 1)
    th = np.full(a.pairs, 4.0)
    calls = [("estimate_homographies", dict(use_mle=mle),
              lambda mle=mle: lib.estimate_homographies(po, f1, f2, th, options=abi.homography_ransac_options(
                  device=0, seed=1, use_mle=mle))) for mle in (0, 1)]
    calls.append(("estimate_uncalibrated_relative_poses", dict(same_batch=True),
                  lambda: lib.estimate_uncalibrated_relative_poses(po, f1, f2, th, options=abi.two_view_ransac_options(
                      device=0, seed=1))))
    for what, extra, call in calls:
        out, med = measure(call, a.repeats)
        s = out["summary"]
        ok = out["status"] == 0
        phases = dict(hypothesis=med[3], score=med[4], replay=med[5])
        line = dict(what=what, **extra, pairs=a.pairs, correspondences=a.correspondences, inlier_ratio=a.inlier_ratio,
                    repeats=a.repeats, wall_seconds_median=med[0], call_seconds_median=med[1],
                    kernel_seconds_median=med[2], kernel_share_of_call=med[2] / med[1] if med[1] else None,
                    hypothesis_seconds_median=med[3], score_seconds_median=med[4], replay_seconds_median=med[5],
                    dominant_kernel=max(phases, key=phases.get), num_chunks=int(s.num_chunks),
                    total_iterations=int(s.total_iterations), total_scores=int(s.total_scores),
                    hypotheses_per_second=s.total_iterations / med[2] if med[2] else None,
                    scores_per_second=s.total_scores / med[2] if med[2] else None, num_estimated=int(s.num_estimated),
                    num_no_model=int(s.num_no_model),
                    median_inlier_share=float(np.median(out["num_inliers"][ok] / a.correspondences)) if ok.any() else None)
        print(json.dumps(line), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
