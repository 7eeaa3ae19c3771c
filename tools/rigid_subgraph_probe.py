"""Device time of tmi_ba_extract_parallel_rigid_subgraph by phase on the generated view graph of the other pose-graph
probes (tools/rotation_nonlinear_probe.py: 1 778 views / 20 000 edges, a spanning chain and random pairs) with exact
relative positions, and on a variant with 50 leaf views hung on it by one edge each (every leaf adds a null direction
and is removed).  The median of --repeats runs after a warm-up.  Appends one JSON line per graph to --out (default
profiles/rigid_subgraph_probe.jsonl): kernel and wall time, the time of the factorisation, the substitution, the graph
kernels (assembly, L Y, Gram-Schmidt, Rayleigh-Ritz, reductions) and the search, the block width, the iteration count
and the null dimension.

    python tools/rigid_subgraph_probe.py [--repeats 3] [--out FILE]

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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rigid_subgraph_model as rsg_model  # noqa: E402
import rotation_nonlinear_model as model  # noqa: E402
from theiasfm_amd import abi, lib  # noqa: E402

VIEWS, PAIRS, LEAVES = 1778, 20000, 50


def scene(num_leaves, rng):
    pairs = model.random_pairs(VIEWS, PAIRS, rng)
    V = VIEWS + num_leaves
    orientation = rng.uniform(-1.0, 1.0, (V, 3))
    position = rng.uniform(-10.0, 10.0, (V, 3))
    pairs += [(int(rng.integers(0, VIEWS)), VIEWS + leaf) for leaf in range(num_leaves)]
    v1 = np.array([p[0] for p in pairs], dtype=np.int32)
    v2 = np.array([p[1] for p in pairs], dtype=np.int32)
    t = position[v2] - position[v1]
    t /= np.linalg.norm(t, axis=1)[:, None]
    R = np.array([rsg_model.angle_axis_to_rotation_matrix(o) for o in orientation])
    return abi.ViewPairBatch(orientation, v1, v2, None, np.einsum("eab,eb->ea", R[v1], t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rigid_subgraph_probe.jsonl"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for what, num_leaves in (("rigid_subgraph", 0), ("rigid_subgraph_with_leaves", LEAVES)):
        batch = scene(num_leaves, np.random.default_rng(1))
        lib.extract_parallel_rigid_subgraph(batch)  # warm-up
        runs = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            out = lib.extract_parallel_rigid_subgraph(batch)
            runs.append((time.perf_counter() - t0, out["summary"]))
        s = out["summary"]
        med = lambda f: float(np.median([f(w, q) for w, q in runs]))  # noqa: E731
        line = dict(what=what, views=batch.num_views, pairs=batch.num_pairs, leaves=num_leaves, order=s.order,
                    repeats=a.repeats, null_dimension=s.null_dimension, block_width=s.block_width, iterations=s.iterations,
                    fixed_view=s.fixed_view, num_kept=s.num_kept, leaves_removed=int((out["keep"][VIEWS:] == 0).sum()),
                    max_residual=s.max_residual, stop_tolerance=s.stop_tolerance,
                    largest_null_value=s.largest_null_value, smallest_other_value=s.smallest_other_value,
                    largest_diagonal=s.largest_diagonal,
                    kernel_seconds_median=med(lambda w, q: q.kernel_seconds), wall_seconds_median=med(lambda w, q: w),
                    call_seconds_median=med(lambda w, q: q.seconds), factor_seconds_median=med(lambda w, q: q.factor_seconds),
                    substitution_seconds_median=med(lambda w, q: q.substitution_seconds),
                    graph_seconds_median=med(lambda w, q: q.graph_seconds),
                    search_seconds_median=med(lambda w, q: q.search_seconds))
        print(json.dumps(line), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
