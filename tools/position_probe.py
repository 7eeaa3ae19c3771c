"""Device time of the LUD position estimator (tmi_ba_estimate_global_positions_lud) on a generated view graph:
1 778 views / 20 000 edges, 2 degrees of noise, 10 % of the non-tree edges replaced by random directions.  The median of
--repeats runs after a warm-up.  Appends one JSON line to --out (default profiles/position_estimator_probe.jsonl):
kernel and wall time, the iteration count and the share of the device time in assembly + factorisation, substitution and
the per-edge / per-view kernels.

    python tools/position_probe.py [--repeats 5] [--max-iterations 1000] [--out FILE]

No time of the reference is given: no Eigen / CHOLMOD build of it exists here.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import position_lud_model as model  # noqa: E402
from theiasfm_amd import abi, lib  # noqa: E402

VIEWS, PAIRS = 1778, 20000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max-iterations", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "position_estimator_probe.jsonl"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    gt, o, v1, v2, p2 = model.make_scene(VIEWS, PAIRS, 2.0, seed=1, outlier_fraction=0.1)
    batch = abi.ViewPairBatch(o, v1, v2, None, p2)
    options = abi.lud_position_options(max_num_iterations=a.max_iterations)
    lib.estimate_global_positions_lud(batch, 0, options)  # warm-up: code object load, allocator
    runs = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        out = lib.estimate_global_positions_lud(batch, 0, options)
        runs.append((time.perf_counter() - t0, out["summary"]))
    s = out["summary"]
    med = lambda f: float(np.median([f(w, r) for w, r in runs]))  # noqa: E731
    kernel = med(lambda w, r: r.kernel_seconds)
    order = 3 * (VIEWS - 1)
    line = dict(what="lud_position", views=VIEWS, pairs=PAIRS, order=order, noise_deg=2.0, outlier_fraction=0.1,
                repeats=a.repeats, max_num_iterations=a.max_iterations, kernel_seconds_median=kernel,
                wall_seconds_median=med(lambda w, r: w), call_seconds_median=med(lambda w, r: r.seconds),
                factor_seconds_median=med(lambda w, r: r.factor_seconds),
                substitution_seconds_median=med(lambda w, r: r.substitution_seconds),
                graph_seconds_median=med(lambda w, r: r.graph_seconds),
                factor_share=med(lambda w, r: r.factor_seconds) / kernel,
                substitution_share=med(lambda w, r: r.substitution_seconds) / kernel,
                graph_kernel_share=med(lambda w, r: r.graph_seconds) / kernel,
                admm_iterations=s.num_admm_iterations, converged=bool(s.converged),
                substitution_launches_per_iteration=2 * ((order + 63) // 64),
                substitution_microseconds_per_launch=1e6 * med(lambda w, r: r.substitution_seconds)
                / (s.num_admm_iterations * 2 * ((order + 63) // 64)),
                smallest_scale=float(out["scales"].min()),
                max_error_after_alignment=float(model.aligned_errors(gt, out["positions"]).max()))
    print(json.dumps(line), flush=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
