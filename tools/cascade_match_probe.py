"""Device time of the batched cascade hashing matcher (tmi_ba_match_features_cascade) beside the brute-force matcher
(tmi_ba_match_features) on the same inputs, the same box and in the same run: --images images of --descriptors
descriptors of --dim elements, all image pairs, the reference's default options, projections from the shim's generator
(synth.cascade_projections at its default seed).  The median of --repeats calls after a warm-up, for each of the two
calls.  Appends one JSON line to --out (default profiles/cascade_match_probe.jsonl).

    python tools/cascade_match_probe.py [--images 8] [--descriptors 8000] [--dim 128] [--repeats 5] [--out FILE]

recall: the share of the brute-force call's matches (pair, feature1, feature2) that the cascade call returns.
mean_candidates_per_row: candidates_examined over the rows of every computed pass (both directions of every pair).
share_of_gather_bound: the bytes the hot kernel has to gather -- 32 B per candidate record examined plus dim * 4 B per
exact distance (the query rows and the CSR entries are left out) -- over kernel_seconds, against the HBM rate.  The
hashing kernels are inside kernel_seconds, so the share understates the hot kernel's own.
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
from theiasfm_amd import abi, lib, synth  # noqa: E402

HBM_BYTES_PER_SECOND = 8.0e12


def timed(call, repeats):
    call()  # warm-up: code object load, allocator
    runs = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = call()
        runs.append((time.perf_counter() - t0, out["summary"].total_seconds, out["summary"].kernel_seconds))
    med = lambda i: float(np.median([r[i] for r in runs]))  # noqa: E731
    return out, dict(kernel_seconds=med(2), call_seconds=med(1), wall_seconds=med(0))


def match_set(out):
    pair = np.repeat(np.arange(out["pair_status"].shape[0]), np.diff(out["pair_match_begin"]))
    return set(zip(pair.tolist(), out["feature1"].tolist(), out["feature2"].tolist()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--descriptors", type=int, default=8000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cascade_match_probe.jsonl"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    begin, desc, _ = synth.make_matching_batch(a.images, a.descriptors, a.dim, seed=1, match_share=0.5, noise=0.03)
    proj = synth.cascade_projections(a.dim)
    p1, p2 = np.triu_indices(a.images, 1)
    cascade, tc = timed(lambda: lib.match_features_cascade(begin, desc, proj, p1, p2,
                                                           options=abi.cascade_match_options(device=0)), a.repeats)
    brute, tb = timed(lambda: lib.match_features(begin, desc, p1, p2, options=abi.match_options(device=0)), a.repeats)
    s = cascade["summary"]
    want, got = match_set(brute), match_set(cascade)
    rows = int(2 * (np.diff(begin)[p1].sum() + np.diff(begin)[p2].sum()) // 2)
    gathered = 32.0 * s.candidates_examined + 4.0 * a.dim * s.distance_evaluations
    line = dict(what="match_features_cascade", box=socket.gethostname(), images=a.images, descriptors=a.descriptors,
                dim=a.dim, pairs=int(p1.shape[0]), repeats=a.repeats, **tc,
                brute_force_kernel_seconds=tb["kernel_seconds"], brute_force_call_seconds=tb["call_seconds"],
                brute_force_wall_seconds=tb["wall_seconds"], num_matches=int(s.num_matches),
                brute_force_num_matches=int(brute["summary"].num_matches),
                recall=(len(want & got) / len(want)) if want else None,
                matches_not_in_brute_force=len(got - want), rows=rows, rows_skipped=int(s.rows_skipped),
                candidates_examined=int(s.candidates_examined), mean_candidates_per_row=s.candidates_examined / max(rows, 1),
                distance_evaluations=int(s.distance_evaluations),
                brute_force_distance_evaluations=int(brute["summary"].distance_evaluations), gathered_bytes=gathered,
                hbm_bytes_per_second=HBM_BYTES_PER_SECOND,
                share_of_gather_bound=(gathered / HBM_BYTES_PER_SECOND / tc["kernel_seconds"]) if tc["kernel_seconds"] > 0 else None,
                num_pairs_ok=int(s.num_pairs_ok), num_chunks=int(s.num_chunks))
    print(json.dumps(line), flush=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
