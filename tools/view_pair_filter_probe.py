"""Kernel time of the 1DSfM translation filter (tmi_ba_filter_view_pairs_from_relative_translation) and of the
orientation filter on generated view graphs: 1 778 views / 20 000 edges and 5 000 views / 100 000 edges, 48 and 256
iterations, the median of --repeats calls after a warm-up.  kernel_seconds is the device time between HIP events around
the call's launches (rotate + moments, then order + sum); seconds is the whole call with uploads and the host's CSR.
Appends one JSON line per measurement to --out (default profiles/view_pair_filter_probe.jsonl).

    python tools/view_pair_filter_probe.py [--repeats 5] [--out FILE]
"""
import argparse
import json
import os
import socket
import sys

import numpy as np
from scipy.spatial.transform import Rotation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from theiasfm_amd import abi, lib  # noqa: E402

SIZES = ((1778, 20000), (5000, 100000))
ITERATIONS = (48, 256)


def make_graph(num_views, num_pairs, seed, outlier_fraction=0.2):
    """Random poses, the path (i, i + 1) plus random further pairs; a fifth of the edges carry a random direction and a
    rotation_2 that is off by up to a radian."""
    rng = np.random.default_rng(seed)
    V = num_views
    aa = rng.uniform(-1, 1, (V, 3))
    pos = rng.uniform(-1, 1, (V, 3)) * V ** (1.0 / 3.0)
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
    R = Rotation.from_rotvec(aa)
    d = pos[v2] - pos[v1]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rot2 = (R[v2] * R[v1].inv()).as_rotvec()
    out = rng.random(len(k)) < outlier_fraction
    r = rng.normal(size=(int(out.sum()), 3))
    d[out] = r / np.linalg.norm(r, axis=1, keepdims=True)
    rot2[out] += rng.uniform(-1, 1, (int(out.sum()), 3))
    return abi.ViewPairBatch(aa, v1, v2, rot2, R[v1].apply(d))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view_pair_filter_probe.jsonl"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("view_pair_filter_probe: no GPU (the probe measures the device; it has no CPU fallback)")
    box = dict(host=socket.gethostname(), device=torch.cuda.get_device_name(0))
    lines = []

    def measure(name, batch, run, extra):
        run()  # warm-up: code object load, allocator
        outs = [run() for _ in range(a.repeats)]
        k = [o[-1].kernel_seconds * 1e3 for o in outs]
        s = [o[-1].seconds * 1e3 for o in outs]
        line = dict(what=name, views=batch.num_views, pairs=batch.num_pairs, kernel_ms_median=float(np.median(k)),
                    kernel_ms_min=float(min(k)), kernel_ms_all=[round(x, 4) for x in k],
                    call_ms_median=float(np.median(s)), pairs_removed=int(outs[-1][-1].num_pairs_removed),
                    **extra, **box)
        lines.append(line)
        print(json.dumps(line), flush=True)

    for views, pairs in SIZES:
        B = make_graph(views, pairs, 7)
        for iterations in ITERATIONS:
            o = abi.translation_filter_options(num_iterations=iterations, seed=3)
            measure("translation_filter", B, lambda: lib.filter_view_pairs_from_relative_translation(B, o),
                    dict(iterations=iterations))
        measure("orientation_filter", B, lambda: lib.filter_view_pairs_from_orientation(B, 5.0), dict(iterations=0))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
