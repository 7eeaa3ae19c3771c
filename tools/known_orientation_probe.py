#!/usr/bin/env python
"""Throughput probe of tmi_ba_estimate_positions_known_orientation (V views of n 2D-3D correspondences) and
tmi_ba_estimate_relative_positions_known_orientation (P view pairs of n correspondences) at a given inlier ratio, under
both scorings (inlier count, MLESAC).  Reports hypotheses per second and correspondence scores per second (over the
call's kernel_seconds, which includes the rotation launches), kernel_seconds against the call, and the hypothesis /
score / replay split from the summary.  Appends one JSON line per call to profiles/known_orientation_probe.jsonl.

  python tools/known_orientation_probe.py [--views 1778] [--pairs 20000] [--correspondences 300] [--inlier-ratio 0.5]
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
THRESHOLD = 16.0 / FOCAL ** 2  # 4 px, squared, normalised units


def rotations_about_y(ang):
    """[N, 3, 3] rotations and their [N, 3] angle-axes."""
    c, s, z, o = np.cos(ang), np.sin(ang), np.zeros_like(ang), np.ones_like(ang)
    R = np.stack([np.stack([c, z, s], -1), np.stack([z, o, z], -1), np.stack([-s, z, c], -1)], -2)
    return R, np.stack([z, ang, z], -1)


def make_batch(kind, items, n, inlier_ratio, pixel_noise, seed):
    """`items` views (absolute) or view pairs (relative) of n correspondences: points in [-2, 2]^2 x [6, 10], a turn of
    up to 0.2 rad about y per view, a position in [-1, 1]^3, the share 1 - inlier_ratio replaced by uniform features."""
    rng = np.random.default_rng(seed)
    X = np.concatenate([rng.uniform(-2.0, 2.0, size=(items, n, 2)), rng.uniform(6.0, 10.0, size=(items, n, 1))], axis=2)
    pos = rng.uniform(-1.0, 1.0, size=(items, 1, 3))
    R2, aa2 = rotations_about_y(rng.uniform(-0.2, 0.2, size=items))
    R1, aa1 = rotations_about_y(rng.uniform(-0.2, 0.2, size=items))
    out = rng.uniform(size=(items, n)) >= inlier_ratio

    def project(R, Y):
        q = np.einsum("pij,pnj->pni", R, Y)
        f = q[..., :2] / q[..., 2:]
        f[out] = rng.uniform(-1.0, 1.0, size=(int(out.sum()), 2))
        return (f + rng.uniform(-pixel_noise, pixel_noise, size=f.shape) / FOCAL).reshape(-1, 2)

    po = np.arange(items + 1, dtype=np.int64) * n
    if kind == "absolute":
        return dict(item_offset=po, feature=project(R2, X - pos), world_point=X.reshape(-1, 3), item_orientation=aa2)
    return dict(pair_offset=po, feature1=project(R1, X), feature2=project(R2, X - pos), pair_orientation1=aa1,
                pair_orientation2=aa2)


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
    ap.add_argument("--views", type=int, default=1778)
    ap.add_argument("--pairs", type=int, default=20000)
    ap.add_argument("--correspondences", type=int, default=300)
    ap.add_argument("--inlier-ratio", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "known_orientation_probe.jsonl"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    batches = {"absolute": (a.views, make_batch("absolute", a.views, a.correspondences, a.inlier_ratio, 0.5, 1)),
               "relative": (a.pairs, make_batch("relative", a.pairs, a.correspondences, a.inlier_ratio, 0.5, 2))}
    fns = {"absolute": lib.estimate_positions_known_orientation,
           "relative": lib.estimate_relative_positions_known_orientation}
    for kind, (items, batch) in batches.items():
        th = np.full(items, THRESHOLD)
        for mle in (0, 1):
            options = abi.known_orientation_ransac_options(device=0, seed=1, use_mle=mle)
            out, med = measure(lambda: fns[kind](*batch.values(), th, options=options), a.repeats)
            s = out["summary"]
            ok = out["status"] == 0
            phases = dict(hypothesis=med[3], score=med[4], replay=med[5])
            line = dict(what=fns[kind].__name__, use_mle=mle, items=items, correspondences=a.correspondences,
                        inlier_ratio=a.inlier_ratio, repeats=a.repeats, wall_seconds_median=med[0],
                        call_seconds_median=med[1], kernel_seconds_median=med[2],
                        kernel_share_of_call=med[2] / med[1] if med[1] else None, hypothesis_seconds_median=med[3],
                        score_seconds_median=med[4], replay_seconds_median=med[5],
                        dominant_kernel=max(phases, key=phases.get), num_chunks=int(s.num_chunks),
                        total_iterations=int(s.total_iterations), total_scores=int(s.total_scores),
                        hypotheses_per_second=s.total_iterations / med[2] if med[2] else None,
                        scores_per_second=s.total_scores / med[2] if med[2] else None,
                        num_estimated=int(s.num_estimated), num_no_model=int(s.num_no_model),
                        median_inlier_share=float(np.median(out["num_inliers"][ok] / a.correspondences)) if ok.any() else None)
            print(json.dumps(line), flush=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
