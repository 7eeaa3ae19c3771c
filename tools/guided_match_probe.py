"""Device time of the batched guided epipolar matcher (tmi_ba_guided_epipolar_match) beside the exact brute-force
matcher (tmi_ba_match_features) on the same image pairs, the same box and in the same run, at the exact matcher's probe
sizes: --images images of --descriptors descriptors of --dim elements, all image pairs, default options.  The images
are views of one synthetic scene (every image sees every 3D point, in an order of its own; keypoints are pinhole
projections plus 0.3 px of noise; descriptors a unit vector per point plus noise); --given of the true matches of a
pair are its input matches, the rest is what guided matching can add.  The median of --repeats calls after a warm-up.

    python tools/guided_match_probe.py [--images 8] [--descriptors 8000] [--dim 128] [--given 0.6] [--repeats 5]

Run on an MI355X it appends one JSON line to --out (default profiles/guided_match_probe.jsonl).  Anywhere else it says
so and claims no time.  Its only comparison is the exact matcher's device time from the same run; the two calls do
different work (the exact matcher looks at every pair of descriptors, both directions), so the ratio says what the
guided step costs beside the matching it follows, not which is faster at one task.
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
from theiasfm_amd import abi, lib  # noqa: E402


def device_arch():
    """The architecture name of device 0 (gfx950 on an MI355X), or None without a device."""
    try:
        import torch
        return torch.cuda.get_device_properties(0).gcnArchName if torch.cuda.is_available() else None
    except Exception:  # noqa: BLE001
        return None


def make_scene(num_images, n, dim, given, seed=1):
    import guided_matching_model as gm
    rng = np.random.default_rng(seed)
    K = np.array([[1600.0, 0, 2000.0], [0, 1600.0, 1500.0], [0, 0, 1.0]])
    X = np.stack([rng.uniform(-4, 4, n), rng.uniform(-3, 3, n), rng.uniform(8, 14, n)], axis=1)
    base = rng.standard_normal((n, dim))
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    begin = np.arange(num_images + 1, dtype=np.int64) * n
    desc = np.zeros((num_images * n, dim), np.float32)
    keys = np.zeros((num_images * n, 2))
    P, feature_of = [], []
    for m in range(num_images):
        w = rng.normal(0, 0.02, 3)
        angle = np.linalg.norm(w)
        A = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / angle
        R = np.eye(3) + np.sin(angle) * A + (1 - np.cos(angle)) * (A @ A)
        t = np.array([np.cos(2 * np.pi * m / num_images), 0.5 * np.sin(2 * np.pi * m / num_images), 0.1 * m])
        P.append(K @ np.concatenate([R, t[:, None]], axis=1))
        x = (P[m] @ np.concatenate([X, np.ones((n, 1))], axis=1).T).T
        order = rng.permutation(n)  # feature order[i] is point i
        keys[begin[m] + order] = x[:, :2] / x[:, 2:3] + rng.normal(0, 0.3, (n, 2))
        desc[begin[m] + order] = (base + rng.normal(0, 0.02, base.shape)).astype(np.float32)
        feature_of.append(order)
    p1, p2 = np.triu_indices(num_images, 1)
    F = np.stack([gm.fundamental_from_projections(P[b], P[a]).reshape(9) for a, b in zip(p1, p2)])
    mb, m1, m2 = [0], [], []
    for a, b in zip(p1, p2):
        pts = rng.permutation(n)[:int(given * n)]
        m1.append(feature_of[a][pts])
        m2.append(feature_of[b][pts])
        mb.append(mb[-1] + len(pts))
    return (begin, desc, keys, p1.astype(np.int32), p2.astype(np.int32), F, np.asarray(mb, np.int64),
            np.concatenate(m1).astype(np.int32), np.concatenate(m2).astype(np.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--descriptors", type=int, default=8000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--given", type=float, default=0.6)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guided_match_probe.jsonl"))
    a = ap.parse_args()
    name = device_arch()
    if name is None or "gfx950" not in name:
        print(f"guided_match_probe: not run on an MI355X (device: {name}); no time is claimed and nothing is written")
        return
    args = make_scene(a.images, a.descriptors, a.dim, a.given)
    begin, desc, p1, p2 = args[0], args[1], args[3], args[4]

    def timed(call):
        call()  # warm-up: code object load, allocator
        runs = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            out = call()
            runs.append((time.perf_counter() - t0, out["summary"].kernel_seconds))
        return out, float(np.median([r[1] for r in runs])), float(np.median([r[0] for r in runs]))

    guided, guided_kernel, guided_wall = timed(
        lambda: lib.guided_epipolar_match(*args, options=abi.guided_match_options(device=0)))
    exact, exact_kernel, exact_wall = timed(lambda: lib.match_features(begin, desc, p1, p2,
                                                                       options=abi.match_options(device=0)))
    s = guided["summary"]
    line = dict(what="guided_epipolar_match", box=socket.gethostname(), device=name, images=a.images,
                descriptors=a.descriptors, dim=a.dim, given=a.given, pairs=int(p1.shape[0]), repeats=a.repeats,
                kernel_seconds=guided_kernel, wall_seconds=guided_wall, num_added=int(s.num_added),
                num_groups=int(s.num_groups), num_candidates=int(s.num_candidates),
                distance_evaluations=int(s.distance_evaluations), exact_matcher_kernel_seconds=exact_kernel,
                exact_matcher_wall_seconds=exact_wall,
                exact_matcher_distance_evaluations=int(exact["summary"].distance_evaluations),
                guided_over_exact_kernel_seconds=(guided_kernel / exact_kernel) if exact_kernel > 0 else None)
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
