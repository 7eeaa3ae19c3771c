"""Kernel time of the batched two-view verification BA (tmi_ba_verify_two_views) on 20 000 generated view pairs, split
per launch (triangulate / solve / accept), with tmi_ba_adjust_two_views on the equivalent pre-compacted batch in the
same process for scale.  Appends one JSON line per measurement to --out (default profiles/two_view_verify_probe.jsonl).

    python tools/two_view_verify_probe.py [--pairs 20000] [--repeats 5] [--out FILE]
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


def compact(B, status, points, pair_status):
    """the survivors of the pairs at status 0, in order: what the solve of the one call reads"""
    keep = (status == 0) & np.repeat(pair_status == 0, np.diff(B.correspondence_ptr))
    ptr = np.concatenate([[0], np.cumsum(np.add.reduceat(np.append(keep, False).astype(np.int64),
                                                         B.correspondence_ptr[:-1]) *
                                         (np.diff(B.correspondence_ptr) > 0))]).astype(np.int64)
    return abi.TwoViewBatch(B.extrinsics1, B.extrinsics2, B.model1, B.model2, B.intrinsics1, B.intrinsics2,
                            B.constant_intrinsics1, B.constant_intrinsics2, ptr, B.features1[keep], B.features2[keep],
                            points[keep])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=20000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "two_view_verify_probe.jsonl"))
    a = ap.parse_args()
    import torch
    box = dict(host=socket.gethostname(), device=torch.cuda.get_device_name(0))
    models = [(m, 0.2) for m in range(5)]
    B, _ = synth.make_two_view_verification_batch(a.pairs, 5, min_corr=31, max_corr=300, models=models,
                                                  free_intrinsics=0.2, outlier_fraction=0.2, roles=False)
    N = int(B.correspondence_ptr[-1])
    lines = []

    def record(name, runs, extra):
        med = lambda k: float(np.median([r[k] for r in runs]))  # noqa: E731
        line = dict(what=name, pairs=B.num_pairs, correspondences=N, repeats=len(runs),
                    **{k + "_median": med(k) for k in runs[0]}, **extra, **box)
        lines.append(line)
        print(json.dumps(line))

    def verify(ba):
        D = B.copy()
        r = lib.verify_two_views(D, abi.two_view_verification_options(bundle_adjustment=ba))
        s = r["summary"]
        return D, r, dict(kernel_ms=s.kernel_seconds * 1e3, triangulate_ms=s.triangulate_kernel_seconds * 1e3,
                          solve_ms=s.solve_kernel_seconds * 1e3, accept_ms=s.accept_kernel_seconds * 1e3,
                          call_ms=s.seconds * 1e3)

    verify(1)  # warm-up: code object load, allocator
    runs = [verify(1) for _ in range(a.repeats)]
    _, r, _ = runs[-1]
    st = r["correspondence_status"]
    record("verify_two_views", [t for _, _, t in runs],
           dict(rejected_fraction=float((st > 0).sum() / max((st >= 0).sum(), 1)),
                correspondence_status_counts={str(k): int((st == k).sum()) for k in np.unique(st)},
                pair_status_counts={str(k): int((r["pair_status"] == k).sum()) for k in np.unique(r["pair_status"])},
                iterations_mean=float(r["iterations"][r["termination"] >= 0].mean()),
                iterations_max=int(r["iterations"].max())))
    # the triangulation alone, and the existing entry point on what it leaves
    T, rt, _ = verify(0)
    S = compact(B, rt["correspondence_status"], T.points, rt["pair_status"])
    lib.adjust_two_views(S.copy())
    ms = []
    for _ in range(a.repeats):
        out = lib.adjust_two_views(S.copy())
        ms.append(dict(kernel_ms=out[-1].kernel_seconds * 1e3, call_ms=out[-1].seconds * 1e3))
    record("adjust_two_views/pre_compacted", ms, dict(compacted_correspondences=int(S.correspondence_ptr[-1]),
                                                     iterations_mean=float(out[1][out[0] >= 0].mean())))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
