"""Device time of the nonlinear rotation estimator (tmi_ba_estimate_global_rotations_nonlinear) on a generated view
graph: 1 778 views / 20 000 edges, relative rotations off by up to 0.03 radians, 10 % of them replaced by random
rotations, started from OrientationsFromMaximumSpanningTree on the device, no view held (the reference's problem).  The
median of --repeats runs after a warm-up.  Appends one JSON line to --out (default
profiles/rotation_nonlinear_probe.jsonl): kernel and wall time, the iteration and factorisation counts, the share of the
device time in the damped copy + factorisation, the substitution and the graph kernels (per-edge, per-view, assembly,
reductions), and beside it the time of tmi_ba_estimate_global_rotations_robust from the same start on the same graph.

    python tools/rotation_nonlinear_probe.py [--repeats 3] [--max-iterations 200] [--out FILE]

No time of the reference is given: no Ceres build of it exists here.
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
import rotation_nonlinear_model as model  # noqa: E402
from theiasfm_amd import abi, lib  # noqa: E402

VIEWS, PAIRS = 1778, 20000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--max-iterations", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rotation_nonlinear_probe.jsonl"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    rng = np.random.default_rng(1)
    gt, v1, v2, rel = model.scene_on_pairs(VIEWS, model.random_pairs(VIEWS, PAIRS, rng), 0.03, 2, 0.1)
    batch = abi.ViewPairBatch(None, v1, v2, rel, None, VIEWS)
    start = lib.orientations_from_maximum_spanning_tree(batch, rng.integers(30, 200, size=PAIRS).astype(np.int32))["orientation"]
    options = abi.nonlinear_rotation_options(max_num_iterations=a.max_iterations)
    lib.estimate_global_rotations_nonlinear(batch, start, abi.nonlinear_rotation_options(max_num_iterations=2))  # warm-up
    runs = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        out = lib.estimate_global_rotations_nonlinear(batch, start, options)
        runs.append((time.perf_counter() - t0, out["summary"]))
    s = out["summary"]
    robust_batch = abi.RelativeRotationBatch(VIEWS, v1, v2, rel)
    lib.estimate_global_rotations_robust(robust_batch, start)  # warm-up
    robust = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        r = lib.estimate_global_rotations_robust(robust_batch, start)
        robust.append((time.perf_counter() - t0, r["summary"]))

    def loop_error(rot):
        return float(np.abs(model.loop_rotations(rot, v1, v2) - model.loop_rotations(gt, v1, v2)).max(axis=(1, 2)).mean())

    med = lambda f, rs=runs: float(np.median([f(w, q) for w, q in rs]))  # noqa: E731
    kernel = med(lambda w, q: q.kernel_seconds)
    factor, subst = med(lambda w, q: q.factor_seconds), med(lambda w, q: q.substitution_seconds)
    line = dict(what="nonlinear_rotation", views=VIEWS, pairs=PAIRS, order=3 * VIEWS, noise_rad=0.03, outlier_fraction=0.1,
                fixed_view=-1, repeats=a.repeats, max_num_iterations=a.max_iterations, kernel_seconds_median=kernel,
                wall_seconds_median=med(lambda w, q: w), call_seconds_median=med(lambda w, q: q.seconds),
                factor_seconds_median=factor, substitution_seconds_median=subst,
                graph_seconds_median=med(lambda w, q: q.graph_seconds), factor_share=factor / kernel,
                substitution_share=subst / kernel, graph_kernel_share=med(lambda w, q: q.graph_seconds) / kernel,
                iterations=s.num_iterations, successful_steps=s.num_successful_steps,
                unsuccessful_steps=s.num_unsuccessful_steps, factorizations=s.num_factorizations,
                termination=s.termination, initial_cost=s.initial_cost, final_cost=s.final_cost,
                factor_milliseconds_per_factorization=1e3 * factor / max(s.num_factorizations, 1),
                substitution_milliseconds_per_iteration=1e3 * subst / max(s.num_factorizations, 1),
                mean_loop_rotation_error_start=loop_error(start), mean_loop_rotation_error_result=loop_error(out["rotations"]),
                robust_wall_seconds_median=med(lambda w, q: w, robust),
                robust_kernel_seconds_median=med(lambda w, q: getattr(q, "kernel_seconds", 0.0), robust),
                mean_loop_rotation_error_robust=loop_error(r["rotations"]))
    print(json.dumps(line), flush=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
