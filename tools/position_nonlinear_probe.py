"""Device time of the nonlinear position estimator (tmi_ba_estimate_global_positions_nonlinear) on a generated view
graph: 1 778 views / 20 000 edges, 2 degrees of noise, 10 % of the non-tree edges replaced by random directions, the
random start of --seed.  The median of --repeats runs after a warm-up.  Appends one JSON line to --out (default
profiles/position_nonlinear_probe.jsonl): kernel and wall time, the iteration and factorisation counts and the share of
the device time in the damped copy + factorisation, the substitution and the graph kernels (per-edge, per-view, assembly,
reductions).

    python tools/position_nonlinear_probe.py [--repeats 3] [--max-iterations 400] [--seed 0] [--out FILE]

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
import position_lud_model as model  # noqa: E402
from theiasfm_amd import abi, lib  # noqa: E402

VIEWS, PAIRS = 1778, 20000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--max-iterations", type=int, default=400)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "position_nonlinear_probe.jsonl"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    gt, o, v1, v2, p2 = model.make_scene(VIEWS, PAIRS, 2.0, seed=1, outlier_fraction=0.1)
    batch = abi.ViewPairBatch(o, v1, v2, None, p2)
    options = abi.nonlinear_position_options(max_num_iterations=a.max_iterations, seed=a.seed)
    warm = abi.nonlinear_position_options(max_num_iterations=2, seed=a.seed)
    lib.estimate_global_positions_nonlinear(batch, 0, warm)  # warm-up: code object load, allocator
    runs = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        out = lib.estimate_global_positions_nonlinear(batch, 0, options)
        runs.append((time.perf_counter() - t0, out["summary"]))
    s = out["summary"]
    med = lambda f: float(np.median([f(w, r) for w, r in runs]))  # noqa: E731
    kernel = med(lambda w, r: r.kernel_seconds)
    factor, subst = med(lambda w, r: r.factor_seconds), med(lambda w, r: r.substitution_seconds)
    line = dict(what="nonlinear_position", views=VIEWS, pairs=PAIRS, order=3 * (VIEWS - 1), noise_deg=2.0,
                outlier_fraction=0.1, seed=a.seed, repeats=a.repeats, max_num_iterations=a.max_iterations,
                kernel_seconds_median=kernel, wall_seconds_median=med(lambda w, r: w),
                call_seconds_median=med(lambda w, r: r.seconds), factor_seconds_median=factor,
                substitution_seconds_median=subst, graph_seconds_median=med(lambda w, r: r.graph_seconds),
                factor_share=factor / kernel, substitution_share=subst / kernel,
                graph_kernel_share=med(lambda w, r: r.graph_seconds) / kernel,
                iterations=s.num_iterations, successful_steps=s.num_successful_steps,
                unsuccessful_steps=s.num_unsuccessful_steps, factorizations=s.num_factorizations,
                termination=s.termination, initial_cost=s.initial_cost, final_cost=s.final_cost,
                factor_milliseconds_per_factorization=1e3 * factor / max(s.num_factorizations, 1),
                substitution_milliseconds_per_iteration=1e3 * subst / max(s.num_factorizations, 1),
                max_error_after_alignment=float(model.aligned_errors(gt, out["positions"]).max()))
    print(json.dumps(line), flush=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
