"""Device time of the robust rotation estimator (tmi_ba_estimate_global_rotations_robust) on generated view graphs:
1 778 views / 20 000 edges and 5 000 views / 100 000 edges, 2 degrees of noise, 10 % of the edges replaced by random
rotations, the chain spanning tree as the start.  The median of --repeats runs after a warm-up.  Appends one JSON line
per graph to --out (default profiles/rotation_estimator_probe.jsonl): kernel and wall time, the iteration counts and the
share of the device time in factorisation, substitution and the per-edge / per-view kernels.

    python tools/rotation_probe.py [--repeats 5] [--model] [--out FILE]

--model also times the numpy model (tests/robust_rotation_model.py) on the CPU on the smaller graph: the model's time,
not the reference's (no Eigen / CHOLMOD build of the reference exists here).
"""
import argparse
import json
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import robust_rotation_model as model  # noqa: E402
from theiasfm_amd import abi, lib  # noqa: E402

GRAPHS = ((1778, 20000), (5000, 100000))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rotation_estimator_probe.jsonl"))
    a = ap.parse_args()
    import torch
    box = dict(host=socket.gethostname(), device=torch.cuda.get_device_name(0))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for views, pairs in GRAPHS:
        gt, v1, v2, rel, o0 = model.make_scene(views, pairs, 2.0, seed=1, outlier_fraction=0.1)
        batch = abi.RelativeRotationBatch(views, v1, v2, rel)
        lib.estimate_global_rotations_robust(batch, o0, 0)  # warm-up: code object load, allocator
        runs = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            out = lib.estimate_global_rotations_robust(batch, o0, 0)
            runs.append((time.perf_counter() - t0, out["summary"]))
        s = out["summary"]
        med = lambda f: float(np.median([f(w, r) for w, r in runs]))  # noqa: E731
        kernel = med(lambda w, r: r.kernel_seconds)
        line = dict(what="robust_rotation", views=views, pairs=pairs, noise_deg=2.0, outlier_fraction=0.1,
                    repeats=a.repeats, kernel_seconds_median=kernel, wall_seconds_median=med(lambda w, r: w),
                    call_seconds_median=med(lambda w, r: r.seconds),
                    factor_share=med(lambda w, r: r.factor_seconds) / kernel,
                    substitution_share=med(lambda w, r: r.substitution_seconds) / kernel,
                    graph_kernel_share=med(lambda w, r: r.graph_seconds) / kernel,
                    l1_iterations=s.num_l1_iterations, admm_iterations=s.num_admm_iterations,
                    admm_per_outer=out["admm_iterations"], irls_iterations=s.num_irls_iterations,
                    factorizations=s.num_factorizations, l1_converged=bool(s.l1_converged),
                    irls_converged=bool(s.irls_converged),
                    max_error_deg_after_alignment=float(model.aligned_errors_deg(gt, out["rotations"]).max()), **box)
        if a.model and views == GRAPHS[0][0]:
            t0 = time.perf_counter()
            ref = model.estimate(views, v1, v2, rel, o0, 0)
            line["model_cpu_seconds"] = time.perf_counter() - t0
            line["model_trace_equal"] = (ref["admm_iterations"] == out["admm_iterations"]
                                         and len(ref["irls_steps"]) == s.num_irls_iterations)
            line["model_rotation_difference_rad"] = float(model.rotation_angles(ref["rotations"], out["rotations"]).max())
        print(json.dumps(line), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
