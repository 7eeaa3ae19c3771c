"""Device time of tmi_ba_build_tracks on a Venice-sized synthetic, beside a single-thread host restatement of the
reference's loop (tools/track_build_host_baseline.cc, compiled here with g++ -O2) on the same input, on the same box
and in the same run; the two must return the same tracks.  Appends one JSON line to --out (default
profiles/track_build_probe.jsonl).

    python tools/track_build_probe.py [--views 1778] [--tracks 1000000] [--observations 5000000] [--window 6]
                                      [--cross 0.01] [--repeats 5] [--no-host] [--out FILE]

The input: --tracks true tracks over --views views with the track lengths synth.py draws (geometric body, a 0.2 %
Pareto tail of 24 to 400 views); a track's views ascend from a random start; every two of its observations fewer than
--window places apart are an edge; a share --cross of the edges has its second endpoint moved to a random observation
(of another view), so oversize components and inconsistent features occur; edges come grouped by view pair, as a
reconstruction builder adds them, in a random orientation.  The caps are the reference's, 2 and 50.
kernel_seconds, call_seconds (summary.seconds) and wall_seconds are medians of --repeats calls after a warm-up;
phase_seconds (nodes, components, cap, output) are the medians of the call's own event pairs.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from theiasfm_amd import abi, lib, synth  # noqa: E402


def make_input(views, tracks, observations, window, cross, seed=1):
    rng = np.random.default_rng(seed)
    k = synth._track_lengths(rng, views, tracks, observations, heavy_tail=0.002)
    begin = np.concatenate([[0], np.cumsum(k)])
    track = np.repeat(np.arange(tracks), k)
    place = np.arange(observations) - begin[track]
    gap = rng.integers(1, 5, observations)  # at most 4 * 400 < views: a track names a view once
    run = np.cumsum(gap)
    view = (rng.integers(0, views, tracks)[track] + run - run[begin[track]]) % views
    order = np.argsort(view, kind="stable")
    first = np.searchsorted(view[order], np.arange(views))
    feature = np.empty(observations, dtype=np.int64)
    feature[order] = np.arange(observations) - first[view[order]]
    a = np.concatenate([np.flatnonzero(place + d < k[track]) for d in range(1, window)])
    b = np.concatenate([np.flatnonzero(place + d < k[track]) + d for d in range(1, window)])
    moved = np.flatnonzero(rng.random(a.shape[0]) < cross)
    target = rng.integers(0, observations, moved.shape[0])
    ok = view[target] != view[a[moved]]
    b[moved[ok]] = target[ok]
    lo, hi = np.minimum(view[a], view[b]), np.maximum(view[a], view[b])
    by_pair = np.argsort(lo * views + hi, kind="stable")
    a, b = a[by_pair], b[by_pair]
    flip = rng.random(a.shape[0]) < 0.5
    a, b = np.where(flip, b, a), np.where(flip, a, b)
    ends = np.stack([a, b], axis=1).reshape(-1)
    return view[ends].astype(np.uint32), feature[ends].astype(np.uint32)


def host_baseline(ev, ef, o, workdir):
    exe = os.path.join(workdir, "track_build_host_baseline")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tools", "track_build_host_baseline.cc")])
    fin, fout = os.path.join(workdir, "in.bin"), os.path.join(workdir, "out.bin")
    with open(fin, "wb") as f:
        np.array([ev.shape[0] // 2], dtype=np.int64).tofile(f)
        np.array([o.min_track_length, o.max_track_length], dtype=np.int32).tofile(f)
        ev.tofile(f)
        ef.tofile(f)
    times = json.loads(subprocess.check_output([exe, fin, fout], text=True))
    with open(fout, "rb") as f:
        nt, no = np.fromfile(f, dtype=np.int64, count=2)
        begin = np.fromfile(f, dtype=np.int64, count=nt + 1)
        ov = np.fromfile(f, dtype=np.uint32, count=no)
        of = np.fromfile(f, dtype=np.uint32, count=no)
    return times, begin, ov, of


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=1778)
    ap.add_argument("--tracks", type=int, default=1000000)
    ap.add_argument("--observations", type=int, default=5000000)
    ap.add_argument("--window", type=int, default=6)
    ap.add_argument("--cross", type=float, default=0.01)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_build_probe.jsonl"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    t0 = time.perf_counter()
    ev, ef = make_input(a.views, a.tracks, a.observations, a.window, a.cross)
    print(f"input: {ev.shape[0] // 2} edges in {time.perf_counter() - t0:.1f} s", flush=True)
    o = abi.track_build_options(device=0)
    out = lib.build_tracks(ev, ef, o)  # warm-up: code object load, allocator
    runs = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        again = lib.build_tracks(ev, ef, o)
        s = again["summary"]
        runs.append([time.perf_counter() - t0, s.seconds, s.kernel_seconds] + list(s.phase_seconds))
        assert all(again[k].tobytes() == out[k].tobytes() for k in ("track_begin", "obs_view", "obs_feature"))
    med = [float(np.median([r[i] for r in runs])) for i in range(7)]
    s = out["summary"]
    line = dict(what="build_tracks", box=socket.gethostname(), views=a.views, true_tracks=a.tracks, window=a.window,
                cross=a.cross, repeats=a.repeats, min_track_length=o.min_track_length, max_track_length=o.max_track_length,
                num_edges=int(ev.shape[0] // 2), kernel_seconds=med[2], call_seconds=med[1], wall_seconds=med[0],
                phase_seconds=dict(nodes=med[3], components=med[4], cap=med[5], output=med[6]),
                **{k: int(getattr(s, k)) for k in ("num_nodes", "num_components", "num_oversize_components",
                                                   "num_replayed_edges", "num_sets", "num_tracks", "num_observations",
                                                   "num_small_tracks", "num_inconsistent_features")})
    if not a.no_host:
        with tempfile.TemporaryDirectory() as workdir:
            times, begin, ov, of = host_baseline(ev, ef, o, workdir)
        line.update(times)
        line["host_returns_the_same_tracks"] = bool(np.array_equal(begin, out["track_begin"]) and
                                                    np.array_equal(ov, out["obs_view"]) and
                                                    np.array_equal(of, out["obs_feature"]))
        line["host_over_call_seconds"] = times["host_seconds"] / med[1] if med[1] > 0 else None
    print(json.dumps(line), flush=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")
    if not a.no_host and not line["host_returns_the_same_tracks"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
