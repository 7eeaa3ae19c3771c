"""Wall and kernel time of the two view-graph calls (tmi_ba_largest_connected_component and
tmi_ba_orientations_from_maximum_spanning_tree) on a generated view graph of 1 778 views / 20 000 edges with seeded
weights: the median of --repeats calls after a warm-up.  kernel_seconds is the device time between HIP events around
the call's launches; seconds is the whole call with its argument checks, uploads and downloads.  The graph is the path
(i, i + 1) plus random further pairs, so it is one component; a second measurement masks a tenth of the edges.
Appends one JSON line per measurement to --out (default profiles/view_graph_probe.jsonl).

    python tools/view_graph_probe.py [--repeats 3] [--out FILE]
"""
import argparse
import json
import os
import socket
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from theiasfm_amd import abi, lib  # noqa: E402

VIEWS, PAIRS = 1778, 20000


def make_graph(num_views, num_pairs, seed):
    rng = np.random.default_rng(seed)
    V = num_views
    keys = {i * V + i + 1 for i in range(V - 1)}
    while len(keys) < num_pairs:
        a = rng.integers(0, V, 2 * num_pairs)
        b = rng.integers(0, V, 2 * num_pairs)
        ok = a < b
        for k in (a[ok].astype(np.int64) * V + b[ok]).tolist():
            if len(keys) == num_pairs:
                break
            keys.add(k)
    k = np.sort(np.fromiter(keys, np.int64))
    v1, v2 = (k // V).astype(np.int32), (k % V).astype(np.int32)
    rot2 = rng.uniform(-1, 1, (len(k), 3))
    weight = rng.integers(30, 2000, size=len(k)).astype(np.int32)  # num_verified_matches: at least the usual minimum
    mask = (rng.random(len(k)) >= 0.1).astype(np.uint8)
    return abi.ViewPairBatch(None, v1, v2, rot2, None, num_views=V), weight, mask


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view_graph_probe.jsonl"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("view_graph_probe: no GPU (the probe measures the device; it has no CPU fallback)")
    box = dict(host=socket.gethostname(), device=torch.cuda.get_device_name(0))
    B, weight, mask = make_graph(VIEWS, PAIRS, 7)
    lines = []

    def measure(name, run, summary, extra):
        run()  # warm-up: code object load, allocator
        sums = [summary(run()) for _ in range(a.repeats)]
        k = [s.kernel_seconds * 1e3 for s in sums]
        w = [s.seconds * 1e3 for s in sums]
        line = dict(what=name, views=B.num_views, pairs=B.num_pairs, kernel_ms_median=float(np.median(k)),
                    kernel_ms_all=[round(x, 4) for x in k], call_ms_median=float(np.median(w)),
                    call_ms_all=[round(x, 4) for x in w], largest_num_views=int(sums[-1].largest_num_views),
                    pairs_kept=int(sums[-1].num_pairs_kept), **extra(), **box)
        lines.append(line)
        print(json.dumps(line), flush=True)

    for label, m in (("all_edges", None), ("tenth_masked", mask)):
        measure("largest_connected_component", lambda: lib.largest_connected_component(B, m), lambda o: o[-1],
                lambda: dict(mask=label))
        last = {}

        def tree():
            last["o"] = lib.orientations_from_maximum_spanning_tree(B, weight, m)
            return last["o"]

        measure("orientations_from_maximum_spanning_tree", tree, lambda o: o["summary"].component,
                lambda: dict(mask=label, tree_pairs=int(last["o"]["summary"].num_tree_pairs),
                             tree_depth=int(last["o"]["summary"].tree_depth)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
