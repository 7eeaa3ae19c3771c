"""Device time of the batched brute-force matcher (tmi_ba_match_features) on a generated batch: --images images of
--descriptors descriptors of --dim elements, all image pairs, the reference's default options.  The median of --repeats
calls after a warm-up.  Appends one JSON line to --out (default profiles/match_probe.jsonl).

    python tools/match_probe.py [--images 8] [--descriptors 8000] [--dim 128] [--repeats 5] [--out FILE]

share_of_fp32_vector_bound: distance evaluations per second (from kernel_seconds) against the fp32 vector bound of an
uncontracted squared difference: 157.3 TFLOP/s is 78.65e12 lane-operations per second counted as FMAs (two FLOP each);
an element pair costs three lane operations (subtract, multiply, add), so the bound is 78.65e12 / 3 = 26.2e12 element
pairs per second, i.e. 26.2e12 / dim distance evaluations per second (packed instructions do two element pairs each at
half that instruction rate, which is the same bound).
numpy_model_*: the numpy fp32 model of the tests on ONE pair of --model-descriptors descriptors on the host CPU --
labelled as what it is, not the reference's time: no build of the reference exists here.
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
from theiasfm_amd import abi, lib, synth  # noqa: E402

FP32_VECTOR_FLOPS = 157.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--descriptors", type=int, default=8000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--model-descriptors", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_probe.jsonl"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    begin, desc, _ = synth.make_matching_batch(a.images, a.descriptors, a.dim, seed=1, match_share=0.5, noise=0.03)
    p1, p2 = np.triu_indices(a.images, 1)
    o = abi.match_options(device=0)
    lib.match_features(begin, desc, p1, p2, options=o)  # warm-up: code object load, allocator
    runs = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        out = lib.match_features(begin, desc, p1, p2, options=o)
        runs.append((time.perf_counter() - t0, out["summary"].total_seconds, out["summary"].kernel_seconds))
    s = out["summary"]
    kernel = float(np.median([r[2] for r in runs]))
    rate = s.distance_evaluations / kernel if kernel > 0 else None
    bound = FP32_VECTOR_FLOPS / 2.0 / 3.0 / a.dim
    line = dict(what="match_features", box=socket.gethostname(), images=a.images, descriptors=a.descriptors, dim=a.dim,
                pairs=int(p1.shape[0]), repeats=a.repeats, kernel_seconds=kernel,
                call_seconds=float(np.median([r[1] for r in runs])), wall_seconds=float(np.median([r[0] for r in runs])),
                distance_evaluations=int(s.distance_evaluations), distance_evaluations_per_second=rate,
                fp32_vector_bound_evaluations_per_second=bound,
                share_of_fp32_vector_bound=(rate / bound) if rate else None, num_matches=int(s.num_matches),
                num_pairs_ok=int(s.num_pairs_ok), num_chunks=int(s.num_chunks))
    if a.model_descriptors > 0:
        import matching_model as mm
        n = min(a.model_descriptors, a.descriptors)
        t0 = time.perf_counter()
        mm.match_pair(desc[:n], desc[begin[1]:begin[1] + n])
        dt = time.perf_counter() - t0
        line["numpy_model_descriptors"] = n
        line["numpy_model_seconds_one_pair"] = dt
        line["numpy_model_distance_evaluations_per_second"] = 2.0 * n * n / dt
    print(json.dumps(line), flush=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
