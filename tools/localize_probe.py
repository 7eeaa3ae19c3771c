"""Device time of the batched view localisation (tmi_ba_localize_views) on a generated batch: --views candidate views
with --correspondences 2D-3D matches each, a fraction --inlier-ratio of them projections with 0.5 pixel noise under a 4
pixel threshold, the others uniform over the image.  The median of --repeats runs after a warm-up, with and without the
view adjustment.  Appends one JSON line to --out (default profiles/localize_probe.jsonl).

    python tools/localize_probe.py [--views 200] [--correspondences 1000] [--inlier-ratio 0.5] [--repeats 5] [--out FILE]

max_position_error is over the localised views against the generating poses.  With the view adjustment it is that of a
least-squares fit over ALL of a view's observations under the options' loss (TRIVIAL by default), outliers included, as
the reference's BundleAdjustView builds it: with gross outliers it is large, and says nothing about the RANSAC.
No time of the reference is given: no build of it exists here.
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
    ap.add_argument("--views", type=int, default=200)
    ap.add_argument("--correspondences", type=int, default=1000)
    ap.add_argument("--inlier-ratio", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "localize_probe.jsonl"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    P = synth.make_localization_batch(a.views, a.correspondences, 1, inlier_ratio=a.inlier_ratio,
                                      num_points=4 * a.correspondences)
    th = P.meta["error_threshold"]
    line = dict(what="localize_views", views=a.views, correspondences=a.correspondences, inlier_ratio=a.inlier_ratio,
                repeats=a.repeats)
    for ba in (0, 1):
        o = abi.localization_options(bundle_adjust_view=ba, seed=1)
        bo = abi.default_options(device=0)
        lib.localize_views(P.copy(), th, options=o, ba_options=bo)  # warm-up: code object load, allocator
        runs = []
        for _ in range(a.repeats):
            Q = P.copy()
            t0 = time.perf_counter()
            out = lib.localize_views(Q, th, options=o, ba_options=bo)
            runs.append((time.perf_counter() - t0, out["summary"].seconds, out["summary"].kernel_seconds))
        s = out["summary"]
        key = "with_ba" if ba else "ransac_only"
        line[key] = dict(wall_seconds_median=float(np.median([r[0] for r in runs])),
                         call_seconds_median=float(np.median([r[1] for r in runs])),
                         kernel_seconds_median=float(np.median([r[2] for r in runs])),
                         num_localized=int(s.num_localized), num_failed_ba=int(s.num_failed_ba),
                         num_chunks=int(s.num_chunks), total_iterations=int(s.total_iterations))
        err = np.abs(Q.extrinsics - P.meta["true_extrinsics"])[out["status"] == 0]
        line[key]["max_position_error"] = float(err[:, :3].max()) if err.size else None
    print(json.dumps(line), flush=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
