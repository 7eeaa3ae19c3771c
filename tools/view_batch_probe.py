"""Batched BundleAdjustView (tmi_ba_adjust_views) at Venice size, the problem bench.py's venice1778_heavy workload
solves (synth.config("venice1778_heavy")), with every point held constant as a localisation round holds them.
Prints one JSON line per measurement:
  full batch    all 1 778 views: default mask (D = 9), intrinsics_to_optimize NONE (D = 6), HUBER width 10, and
                shared groups of 8 views with free intrinsics (chains of 8 run in sequence by contract);
  small batch   the first 1, 10 and 100 views (view_mask);
  baseline      the same first 100 views through the per-view path (tmi_ba_solve on each one-view problem, DENSE_QR,
                no inner iterations), in the same process.
usage: python tools/view_batch_probe.py"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from theiasfm_amd import abi, lib, synth  # noqa: E402


def options(**kw):
    kw.setdefault("linear_solver_type", abi.DENSE_QR)
    kw.setdefault("use_inner_iterations", 0)
    return abi.default_options(**kw)


def shared_groups(P, size):
    """groups of `size` consecutive views, each with the intrinsics of its first view"""
    n = P.num_cameras
    grp = np.arange(n, dtype=np.int32) // size
    G = int(grp.max()) + 1
    model, off, intr, const = [], [0], [], []
    for g in range(G):
        c = g * size
        og = int(P.camera_group[c])
        a, b = int(P.group_offset[og]), int(P.group_offset[og + 1])
        model.append(int(P.group_model[og]))
        intr.append(P.intrinsics[a:b])
        const.append(P.intrinsics_constant[a:b])
        off.append(off[-1] + b - a)
    return abi.Problem(P.extrinsics.copy(), grp, P.camera_flags.copy(), np.array(model), np.array(off),
                       np.concatenate(intr), np.concatenate(const), P.points.copy(), P.point_constant.copy(),
                       P.obs_camera.copy(), P.obs_point.copy(), P.obs_xy.copy())


def batch(tag, P, opts, mask=None, reps=3):
    walls, kern, call = [], [], []
    for _ in range(reps):
        Q = P.copy()
        t0 = time.perf_counter()
        term, iters, c0, c1, s = lib.adjust_views(Q, opts, mask)
        walls.append(time.perf_counter() - t0)
        kern.append(s.kernel_seconds)
        call.append(s.seconds)
    i = int(np.argmin(walls))
    # host_and_upload_ms: the call's time outside the kernel -- the host passes over all observations, the gather of
    # the selected views' observations, the uploads and the allocations
    out = dict(case=tag, views=int(s.num_views), success=int(s.num_success), chains=int(s.num_chains),
               wall_ms=round(1e3 * walls[i], 3), kernel_ms=round(1e3 * kern[i], 3),
               host_and_upload_ms=round(1e3 * (call[i] - kern[i]), 3),
               mean_iterations=round(s.total_iterations / max(1, s.num_views), 3),
               obs=int(np.isin(P.obs_camera, np.flatnonzero(mask) if mask is not None else np.arange(P.num_cameras)).sum()))
    print(json.dumps(out), flush=True)
    return out


def per_view_loop(P, opts, n):
    Q = P.copy()
    order = np.argsort(Q.obs_camera, kind="stable")
    starts = np.searchsorted(Q.obs_camera[order], np.arange(Q.num_cameras + 1))
    t0 = time.perf_counter()
    its = 0
    for c in range(n):
        obs = order[starts[c]:starts[c + 1]]
        g = int(Q.camera_group[c])
        a, b = int(Q.group_offset[g]), int(Q.group_offset[g + 1])
        pts, inv = np.unique(Q.obs_point[obs], return_inverse=True)
        sub = abi.Problem(Q.extrinsics[c:c + 1].copy(), np.zeros(1, np.int32), Q.camera_flags[c:c + 1].copy(),
                          Q.group_model[g:g + 1].copy(), np.array([0, b - a], np.int32), Q.intrinsics[a:b].copy(),
                          Q.intrinsics_constant[a:b].copy(), Q.points[pts], np.ones(len(pts), np.uint8),
                          np.zeros(len(obs), np.int32), inv.astype(np.int32), Q.obs_xy[obs])
        st, s = lib.solve(sub, opts)
        its += s.num_iterations
        if s.success:
            Q.extrinsics[c] = sub.extrinsics[0]
            Q.intrinsics[a:b] = sub.intrinsics
    dt = time.perf_counter() - t0
    out = dict(case=f"per-view loop, first {n} views (tmi_ba_solve each)", views=n, wall_ms=round(1e3 * dt, 3),
               ms_per_view=round(1e3 * dt / n, 3), mean_iterations=round(its / n, 3))
    print(json.dumps(out), flush=True)
    return out


def main():
    P = synth.config("venice1778_heavy")
    print(json.dumps(dict(problem="venice1778_heavy", cameras=P.num_cameras, points=P.num_points,
                          observations=P.num_observations,
                          obs_per_view_mean=round(P.num_observations / P.num_cameras, 1))), flush=True)
    lib.adjust_views(P.copy(), options(), np.eye(1, P.num_cameras, 0, dtype=np.uint8)[0])  # warm-up: module load
    o = options()
    full = batch("full batch, default mask (D = 9)", P, o)
    Pn = P.copy()
    Pn.set_intrinsics_to_optimize(abi.INTRINSICS_NONE)
    batch("full batch, intrinsics NONE (D = 6)", Pn, o)
    batch("full batch, HUBER width 10", P, options(loss_function_type=abi.LOSS_HUBER, robust_loss_width=10.0))
    batch("full batch, shared groups of 8 with free intrinsics (chains of 8)", shared_groups(P, 8), o)
    small = {}
    for n in (1, 10, 100):
        m = np.zeros(P.num_cameras, np.uint8)
        m[:n] = 1
        small[n] = batch(f"batch of the first {n} views", P, o, m)
    loop = per_view_loop(P, o, 100)
    print(json.dumps(dict(case="speed-up, 100 views", per_view_loop_over_batch=round(loop["wall_ms"] / small[100]["wall_ms"], 1),
                          full_batch_kernel_ms=full["kernel_ms"])), flush=True)


if __name__ == "__main__":
    main()
