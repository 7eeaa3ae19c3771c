"""Batched TrackEstimator (tmi_ba_estimate_tracks) at Venice size: the problem bench.py's venice1778_heavy workload
solves (synth.config("venice1778_heavy")), with the 1DSfM settings of the global pipeline's retriangulation
(min_triangulation_angle_degrees 4, max_acceptable_reprojection_error_pixels 10), track BA on and off.
Prints one JSON line per measurement:
  all tracks    every track selected (its input point is ignored);
  25 %          a seeded quarter of the tracks selected, their points scrambled first;
  cpu sample    the CPU restatement (tests/track_estimator_model.py: per-observation undistortion, pair scan,
                midpoint, oracle.adjust_tracks, acceptance) on a seeded sample of tracks, for scale: ms per track.
usage: python tools/track_estimate_probe.py"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from theiasfm_amd import abi, lib, synth  # noqa: E402

MIN_ANGLE, MAX_ERROR = 4.0, 10.0


def ba_options():
    return abi.default_options(linear_solver_type=abi.DENSE_QR, use_inner_iterations=0)


def run(tag, P, ba, mask=None, reps=3):
    eo = abi.track_estimator_options(max_acceptable_reprojection_error_pixels=MAX_ERROR,
                                     min_triangulation_angle_degrees=MIN_ANGLE, bundle_adjustment=ba)
    walls, kern, call = [], [], []
    for _ in range(reps):
        Q = P.copy()
        t0 = time.perf_counter()
        status, s = lib.estimate_tracks(Q, eo, ba_options(), mask)
        walls.append(time.perf_counter() - t0)
        kern.append(s.kernel_seconds)
        call.append(s.seconds)
    i = int(np.argmin(walls))
    out = dict(case=tag, bundle_adjustment=ba, attempts=int(s.num_attempts), estimated=int(s.num_estimated),
               bad_angle=int(s.num_bad_angle), failed_triangulation=int(s.num_failed_triangulation),
               failed_ba=int(s.num_failed_ba), bad_reprojection=int(s.num_bad_reprojection),
               wall_ms=round(1e3 * walls[i], 3), kernel_ms=round(1e3 * kern[i], 3),
               host_and_upload_ms=round(1e3 * (call[i] - kern[i]), 3))
    print(json.dumps(out), flush=True)
    return out


def cpu_sample(P, ba, n, seed=5):
    """the CPU restatement on n seeded tracks (all their observations, every camera)"""
    import track_estimator_model as model
    rng = np.random.default_rng(seed)
    tracks = np.sort(rng.choice(P.num_points, n, replace=False))
    keep = np.isin(P.obs_point, tracks)
    remap = np.full(P.num_points, -1, np.int32)
    remap[tracks] = np.arange(n, dtype=np.int32)
    sub = abi.Problem(P.extrinsics, P.camera_group, P.camera_flags, P.group_model, P.group_offset, P.intrinsics,
                      P.intrinsics_constant, P.points[tracks], P.point_constant[tracks], P.obs_camera[keep],
                      remap[P.obs_point[keep]], P.obs_xy[keep])
    eo = abi.track_estimator_options(max_acceptable_reprojection_error_pixels=MAX_ERROR,
                                     min_triangulation_angle_degrees=MIN_ANGLE, bundle_adjustment=ba)
    t0 = time.perf_counter()
    status, _ = model.estimate(sub, eo, ba_options())
    dt = time.perf_counter() - t0
    out = dict(case=f"cpu restatement, {n} sampled tracks (python + C oracle)", bundle_adjustment=ba,
               estimated=int((status == 0).sum()), wall_ms=round(1e3 * dt, 3), ms_per_track=round(1e3 * dt / n, 4),
               observations=int(keep.sum()))
    print(json.dumps(out), flush=True)
    return out


def main():
    P = synth.config("venice1778_heavy")
    print(json.dumps(dict(problem="venice1778_heavy", cameras=P.num_cameras, points=P.num_points,
                          observations=P.num_observations, min_angle_degrees=MIN_ANGLE,
                          max_error_pixels=MAX_ERROR)), flush=True)
    warm = np.zeros(P.num_points, np.uint8)
    warm[0] = 1
    lib.estimate_tracks(P.copy(), abi.track_estimator_options(), ba_options(), warm)  # warm-up: module load
    for ba in (1, 0):
        run("all tracks", P, ba)
    rng = np.random.default_rng(3)
    mask = (rng.random(P.num_points) < 0.25).astype(np.uint8)
    Q = P.copy()
    Q.points[mask == 1] = rng.normal(0, 50.0, (int(mask.sum()), 4))
    for ba in (1, 0):
        run("25 % of the tracks, points scrambled", Q, ba, mask)
    for ba in (1, 0):
        cpu_sample(P, ba, 2000)


if __name__ == "__main__":
    main()
