"""Device time of the linear rotation estimator (tmi_ba_estimate_global_rotations_linear) on the generated view graph
of tools/rotation_nonlinear_probe.py: 1 778 views / 20 000 edges, relative rotations off by up to 0.03 radians, 10 % of
them replaced by random rotations.  The median of --repeats runs after a warm-up.  Appends one JSON line to --out
(default profiles/rotation_linear_probe.jsonl): kernel and wall time, the iteration count, the share of the device time
in the factorisation, the substitution and the graph kernels (assembly, M Q, Gram-Schmidt, Rayleigh-Ritz, reductions,
projection), and beside it, in the same process on the same graph, the times of
tmi_ba_estimate_global_rotations_robust and tmi_ba_estimate_global_rotations_nonlinear started from
OrientationsFromMaximumSpanningTree, and of the nonlinear call started from the linear result.

    python tools/rotation_linear_probe.py [--repeats 3] [--max-iterations 1000] [--out FILE]

No time of the reference is given: no Spectra build of it exists here.
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
    ap.add_argument("--max-iterations", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rotation_linear_probe.jsonl"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    rng = np.random.default_rng(1)
    gt, v1, v2, rel = model.scene_on_pairs(VIEWS, model.random_pairs(VIEWS, PAIRS, rng), 0.03, 2, 0.1)
    batch = abi.ViewPairBatch(None, v1, v2, rel, None, VIEWS)
    tree = lib.orientations_from_maximum_spanning_tree(batch, rng.integers(30, 200, size=PAIRS).astype(np.int32))["orientation"]
    options = abi.linear_rotation_options(max_iterations=a.max_iterations)

    def timed(call):
        call()  # warm-up
        runs = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            out = call()
            runs.append((time.perf_counter() - t0, out["summary"]))
        return out, runs

    out, runs = timed(lambda: lib.estimate_global_rotations_linear(batch, options))
    s = out["summary"]
    robust_batch = abi.RelativeRotationBatch(VIEWS, v1, v2, rel)
    r, robust = timed(lambda: lib.estimate_global_rotations_robust(robust_batch, tree))
    nl, nonlinear = timed(lambda: lib.estimate_global_rotations_nonlinear(batch, tree, want_outputs=False))
    nl2, seeded = timed(lambda: lib.estimate_global_rotations_nonlinear(batch, out["rotations"], want_outputs=False))

    def loop_error(rot):
        return float(np.abs(model.loop_rotations(rot, v1, v2) - model.loop_rotations(gt, v1, v2)).max(axis=(1, 2)).mean())

    med = lambda f, rs=runs: float(np.median([f(w, q) for w, q in rs]))  # noqa: E731
    kernel = med(lambda w, q: q.kernel_seconds)
    factor, subst = med(lambda w, q: q.factor_seconds), med(lambda w, q: q.substitution_seconds)
    graph = med(lambda w, q: q.graph_seconds)
    line = dict(what="linear_rotation", views=VIEWS, pairs=PAIRS, order=3 * VIEWS, noise_rad=0.03, outlier_fraction=0.1,
                repeats=a.repeats, max_iterations=a.max_iterations, tolerance=options.tolerance,
                relative_shift=options.relative_shift, kernel_seconds_median=kernel,
                wall_seconds_median=med(lambda w, q: w), call_seconds_median=med(lambda w, q: q.seconds),
                factor_seconds_median=factor, substitution_seconds_median=subst, graph_seconds_median=graph,
                factor_share=factor / kernel, substitution_share=subst / kernel, graph_kernel_share=graph / kernel,
                iterations=s.num_iterations, converged=s.converged, usable=s.usable, num_reflected=s.num_reflected,
                eigenvalues=list(s.eigenvalue), residuals=list(s.residual),
                substitution_milliseconds_per_iteration=1e3 * subst / max(s.num_iterations, 1),
                graph_milliseconds_per_iteration=1e3 * graph / max(s.num_iterations, 1),
                mean_loop_rotation_error_linear=loop_error(out["rotations"]),
                mean_loop_rotation_error_tree=loop_error(tree),
                robust_wall_seconds_median=med(lambda w, q: w, robust),
                mean_loop_rotation_error_robust=loop_error(r["rotations"]),
                nonlinear_from_tree_wall_seconds_median=med(lambda w, q: w, nonlinear),
                nonlinear_from_tree_iterations=nl["summary"].num_iterations,
                mean_loop_rotation_error_nonlinear_from_tree=loop_error(nl["rotations"]),
                nonlinear_from_linear_wall_seconds_median=med(lambda w, q: w, seeded),
                nonlinear_from_linear_iterations=nl2["summary"].num_iterations,
                mean_loop_rotation_error_nonlinear_from_linear=loop_error(nl2["rotations"]))
    print(json.dumps(line), flush=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
