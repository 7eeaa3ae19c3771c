"""CPU restatement of TrackEstimator::EstimateTrack (estimate_track.cc:205-264) for the device tests.

Per selected track, on a flattened problem whose cameras all count as estimated views:
  1. fewer than 2 observations -> 1
  2. rays R^T PixelToCameraCoordinates(pixel), normalized (camera.cc:215-223): oracle.pixel_to_camera and
     ceres::AngleAxisToRotationMatrix restated below
  3. SufficientTriangulationAngle (triangulation.cc:236-250) -> 1 when no pair qualifies
  4. TriangulateMidpoint (triangulation.cc:130-157) with Eigen's unblocked LLT (pivot <= 0 fails) -> 2
  5. BundleAdjustTrack through oracle.adjust_tracks on the surviving tracks -> 3 unless CONVERGENCE / NO_CONVERGENCE
  6. AcceptableReprojectionError (estimate_track.cc:90-115) with oracle.project_point -> 4
  else 0.  Status -1: not selected or a constant point."""
from __future__ import annotations

import math

import numpy as np

from oracle import oracle

DBL_EPSILON = np.finfo(np.float64).eps


def angle_axis_to_rotation_matrix(aa):
    """ceres::AngleAxisToRotationMatrix (Ceres 1.x rotation.h), R[r, c], with its first-order branch."""
    aa = np.asarray(aa, dtype=np.float64)
    theta2 = aa[0] * aa[0] + aa[1] * aa[1] + aa[2] * aa[2]
    R = np.zeros((3, 3))
    if theta2 > DBL_EPSILON:
        theta = math.sqrt(theta2)
        wx, wy, wz = aa[0] / theta, aa[1] / theta, aa[2] / theta
        c, s = math.cos(theta), math.sin(theta)
        omc = 1.0 - c
        R[0, 0] = c + wx * wx * omc
        R[1, 0] = wz * s + wx * wy * omc
        R[2, 0] = -wy * s + wx * wz * omc
        R[0, 1] = wx * wy * omc - wz * s
        R[1, 1] = c + wy * wy * omc
        R[2, 1] = wx * s + wy * wz * omc
        R[0, 2] = wy * s + wx * wz * omc
        R[1, 2] = -wx * s + wy * wz * omc
        R[2, 2] = c + wz * wz * omc
    else:
        R[:] = [[1.0, -aa[2], aa[1]], [aa[2], 1.0, -aa[0]], [-aa[1], aa[0], 1.0]]
    return R


def camera_intrinsics(P, cam):
    g = int(P.camera_group[cam])
    return int(P.group_model[g]), P.intrinsics[P.group_offset[g]:P.group_offset[g + 1]]


def observation_rays(P):
    """[No, 3]: Camera::PixelToUnitDepthRay(pixel).normalized() of every observation."""
    rays = np.zeros((P.num_observations, 3))
    for c in range(P.num_cameras):
        idx = np.flatnonzero(P.obs_camera == c)
        if idx.size == 0:
            continue
        model, K = camera_intrinsics(P, c)
        u = oracle.pixel_to_camera_batch(model, K, P.obs_xy[idx])
        R = angle_axis_to_rotation_matrix(P.extrinsics[c, 3:])
        for n, o in enumerate(idx):
            r = np.array([R[0, i] * u[n, 0] + R[1, i] * u[n, 1] + R[2, i] * u[n, 2] for i in range(3)])
            n2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2]
            rays[o] = r / math.sqrt(n2) if n2 > 0.0 else r
    return rays


def sufficient_angle(rays, min_angle_degrees):
    cos_min = math.cos(min_angle_degrees * math.pi / 180.0)
    for i in range(len(rays)):
        for j in range(i + 1, len(rays)):
            if rays[i][0] * rays[j][0] + rays[i][1] * rays[j][1] + rays[i][2] * rays[j][2] < cos_min:
                return True
    return False


def triangulate_midpoint(origins, dirs):
    """TriangulateMidpoint: 4 x 4 homogeneous normal equations and Eigen's LLT; None where the LLT fails."""
    A = np.zeros((4, 4))
    b = np.zeros(4)
    for o, d in zip(origins, dirs):
        dh = np.array([d[0], d[1], d[2], 0.0])
        T = np.eye(4) - np.outer(dh, dh)
        A += T
        oh = np.array([o[0], o[1], o[2], 1.0])
        b += np.array([((T[r, 0] * oh[0] + T[r, 1] * oh[1]) + T[r, 2] * oh[2]) + T[r, 3] * oh[3] for r in range(4)])
    L = np.zeros((4, 4))
    for k in range(4):  # llt_inplace::unblocked (lower)
        x = A[k, k] - sum(L[k, m] * L[k, m] for m in range(k))
        if x <= 0.0:
            return None
        L[k, k] = math.sqrt(x)
        for r in range(k + 1, 4):
            L[r, k] = (A[r, k] - sum(L[r, m] * L[k, m] for m in range(k))) / L[k, k]
    y = np.zeros(4)
    for i in range(4):
        y[i] = (b[i] - sum(L[i, m] * y[m] for m in range(i))) / L[i, i]
    X = np.zeros(4)
    for i in range(3, -1, -1):
        X[i] = (y[i] - sum(L[m, i] * X[m] for m in range(i + 1, 4))) / L[i, i]
    return X


def estimate(P, estimator_options, ba_options, track_mask=None):
    """(status [Np] int8, points [Np, 4]) of the batched TrackEstimator on P (P itself is not changed)."""
    n = P.num_points
    status = np.full(n, -1, dtype=np.int8)
    points = P.points.copy()
    rays = observation_rays(P)
    order = np.argsort(P.obs_point, kind="stable")
    starts = np.searchsorted(P.obs_point[order], np.arange(n + 1))
    for t in range(n):
        if (track_mask is not None and not track_mask[t]) or P.point_constant[t]:
            continue
        obs = order[starts[t]:starts[t + 1]]
        if len(obs) < 2 or not sufficient_angle(rays[obs], estimator_options.min_triangulation_angle_degrees):
            status[t] = 1
            continue
        X = triangulate_midpoint(P.extrinsics[P.obs_camera[obs], :3], rays[obs])
        if X is None:
            status[t] = 2
            continue
        points[t] = X
        status[t] = 0
    if estimator_options.bundle_adjustment:
        Q = P.copy()
        Q.points[:] = points
        Q.point_constant[:] = (status != 0).astype(np.uint8)
        term, _, _, _ = oracle.adjust_tracks(Q, ba_options)
        ok = status == 0
        status[ok & (term != 0) & (term != 1)] = 3
        points[ok] = Q.points[ok]
    max_sq = estimator_options.max_acceptable_reprojection_error_pixels ** 2
    for t in np.flatnonzero(status == 0):
        obs = order[starts[t]:starts[t + 1]]
        total = 0.0
        behind = False
        for o in obs:
            cam = int(P.obs_camera[o])
            model, K = camera_intrinsics(P, cam)
            px, depth = oracle.project_point(model, P.extrinsics[cam], K, points[t])
            if depth < 0:
                behind = True
                break
            total += float(np.sum((P.obs_xy[o] - px) ** 2))
        if behind or not (total / len(obs) < max_sq):
            status[t] = 4
    return status, points
