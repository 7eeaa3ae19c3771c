"""Kernel time of the batched OptimizeRelativePositionWithKnownRotation (tmi_ba_optimize_relative_positions) on 20 000
generated view-graph edges, with the batched BundleAdjustTwoViewsAngular on the same box in the same run for scale.
Appends one JSON line per measurement to --out (default profiles/relative_position_probe.jsonl).

    python tools/relative_position_probe.py [--pairs 20000] [--repeats 5] [--out FILE]
"""
import argparse
import json
import os
import socket
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from theiasfm_amd import abi, lib, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=20000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relative_position_probe.jsonl"))
    a = ap.parse_args()
    import torch
    box = dict(host=socket.gethostname(), device=torch.cuda.get_device_name(0))
    lines = []

    def measure(name, batch, run, extra):
        run(batch.copy())  # warm-up: code object load, allocator
        ms = []
        for _ in range(a.repeats):
            out = run(batch.copy())
            ms.append(out[-1].kernel_seconds * 1e3)
        n = int(batch.correspondence_ptr[-1])
        line = dict(what=name, pairs=batch.num_pairs, correspondences=n, kernel_ms_median=float(np.median(ms)),
                    kernel_ms_min=float(min(ms)), kernel_ms_all=[round(x, 4) for x in ms],
                    iterations_mean=float(np.mean(out[1])), iterations_max=int(np.max(out[1])), **extra(out), **box)
        lines.append(line)
        print(json.dumps(line))

    rel_extra = lambda o: dict(status_counts={str(k): int((o[0] == k).sum()) for k in np.unique(o[0])})  # noqa: E731
    B, _ = synth.make_relative_position_batch(a.pairs, 5, min_corr=30, max_corr=300, pixel_noise=0.5)
    measure("relative_position/normalised", B, lib.optimize_relative_positions, rel_extra)
    models = [(m, 0.2) for m in range(5)]
    Bp, _ = synth.make_relative_position_batch(a.pairs, 5, min_corr=30, max_corr=300, pixel_noise=0.5, models=models)
    measure("relative_position/pixels", Bp, lib.optimize_relative_positions, rel_extra)
    Bl, _ = synth.make_relative_position_batch(a.pairs // 10, 6, min_corr=513, max_corr=2500, pixel_noise=0.5)
    measure("relative_position/normalised_long", Bl, lib.optimize_relative_positions, rel_extra)
    A, _, _ = synth.make_two_view_angular_batch(a.pairs, 5, max_corr=300)
    measure("two_view_angular", A, lib.adjust_two_views_angular,
            lambda o: dict(status_counts={str(k): int((o[0] == k).sum()) for k in np.unique(o[0])}))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
