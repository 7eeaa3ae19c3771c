"""CPU restatement of TwoViewMatchGeometricVerification::BundleAdjustRelativePose
(two_view_match_geometric_verification.cc:256-324) with the two tests VerifyMatches puts around it, for the device tests.

Per pair with n correspondences (steps as in include/theia_mi355_ba.h, tmi_ba_verify_two_views):
  1. n <= min_num_inlier_matches (:171-176, :181)                          -> pair status 1, correspondences stay -1
  2. TriangulatePoints (:185-254) per correspondence: rays R^T PixelToCameraCoordinates(pixel), normalized
     (oracle.pixel_to_camera_batch and track_estimator_model.angle_axis_to_rotation_matrix); dot < cos(min angle)
     or status 1; track_estimator_model.triangulate_midpoint over {C1, C2} or status 2; AcceptableReprojectionError
     (:72-83, oracle.project_point) in camera 1 and then camera 2 or status 3; survivors keep their order
  3. survivors < min_num_inlier_matches (:268)                             -> pair status 2
  4. BundleAdjustTwoViews through oracle.adjust_two_views on the survivors; termination not 0 / 1 -> pair status 3
  5. the same two-camera test with final_max_reprojection_error (:295-314) -> correspondence status 4
  6. count > min_num_inlier_matches (:181) -> pair status 0, else 4

Every correspondence also gets its MARGIN to the thresholds it was tested against: |dot - cos_min| for the angle and
|err^2 - max^2| / max^2 for every reprojection test that got as far as comparing an error (inf where none did).  A
device result may differ from the model only where that margin is tiny."""
from __future__ import annotations

import math

import numpy as np

from oracle import oracle
from theiasfm_amd import abi
from track_estimator_model import angle_axis_to_rotation_matrix, triangulate_midpoint


K_PLAIN = np.array([800.0, 1.0, 0.0, 500.0, 400.0, 0.0, 0.0, 0.0, 0.0, 0.0])
E2_SIDE = np.array([1.0, 0.05, -0.02, 0.02, -0.06, 0.01])   # a baseline to the right, a small rotation
E2_FACING = np.array([0.0, 0.0, 10.0, np.pi, 0.0, 0.0])     # on camera 1's axis, looking back at it


# ---- constructed pairs (plain pinhole cameras, exact pixels) -----------------------------------
def points(rng, n, depth=(4.0, 7.0)):
    z = rng.uniform(*depth, n)
    return np.concatenate([rng.uniform(-0.2, 0.2, (n, 2)) * z[:, None] + [0.5, 0.0], z[:, None], np.ones((n, 1))], 1)


def pair(e2, X, shift2=None):
    """One pair of plain pinhole cameras and the exact pixels of the points X in both; shift2 [n, 2] moves feature 2."""
    e1 = np.zeros(6)
    f1 = np.array([oracle.project_point(abi.PINHOLE, e1, K_PLAIN, x)[0] for x in X]).reshape(-1, 2)
    f2 = np.array([oracle.project_point(abi.PINHOLE, e2, K_PLAIN, x)[0] for x in X]).reshape(-1, 2)
    if shift2 is not None:
        f2 = f2 + shift2
    return e1, e2.copy(), f1, f2


def batch(pairs):
    ptr = np.concatenate([[0], np.cumsum([p[2].shape[0] for p in pairs])]).astype(np.int64)
    P = len(pairs)
    cat = lambda i, w: np.concatenate([p[i].reshape(-1, w) for p in pairs] + [np.zeros((0, w))])  # noqa: E731
    N = int(ptr[-1])
    return abi.TwoViewBatch(cat(0, 6), cat(1, 6), np.zeros(P, np.int32), np.zeros(P, np.int32), np.tile(K_PLAIN, (P, 1)),
                            np.tile(K_PLAIN, (P, 1)), np.ones(P, np.uint8), np.ones(P, np.uint8), ptr, cat(2, 2),
                            cat(3, 2), np.zeros((N, 4)))


def mixed_pair(rng, n_in, n_far=0, n_near=0, n_gross=0, n_behind=0):
    """n_in exact inliers, then far points (status 1), near misses 20 px across the epipolar lines (they pass the 15 px
    test of the triangulation with about 10 px in each image and fail the 5 px test after the adjustment: status 4),
    gross mismatches and points behind both cameras (status 3)."""
    X = np.concatenate([points(rng, n_in), points(rng, n_far, (400.0, 600.0)), points(rng, n_near),
                        points(rng, n_gross), points(rng, n_behind) * [1, 1, -1, 1]])
    shift = np.zeros((len(X), 2))
    a = n_in + n_far
    shift[a:a + n_near] = [0.0, 20.0]
    shift[a + n_near:a + n_near + n_gross] = [30.0, 250.0]
    kinds = np.repeat([0, 1, 4, 3, 3], [n_in, n_far, n_near, n_gross, n_behind])
    return pair(E2_SIDE, X, shift), kinds


def noisy(pr, rng, sigma=0.3):
    """the pair with Gaussian pixel noise on both features (so that its adjustment has something to do)"""
    e1, e2, f1, f2 = pr
    return e1, e2, f1 + sigma * rng.normal(size=f1.shape), f2 + sigma * rng.normal(size=f2.shape)


def failing_start_pair(rng, n=40):
    """A pair of cameras facing each other whose adjustment fails at its start point (pair status 3): n ordinary exact
    correspondences between them, and correspondence 3 the exact pixels of a point 5e-5 in front of camera 1's centre,
    10 degrees off the common axis.  Its rays meet there (they pass the angle test, the midpoint lands on the point,
    both reprojections are exact with a positive depth), and |X - C1|^2 < 1e-8 fails the residual functor
    (reprojection_error.h:75-77): termination 3."""
    X = points(rng, n, (3.0, 7.0)) - [0.5, 0, 0, 0]
    t = 5e-5
    X[3] = [t * math.sin(math.radians(10.0)), 0.0, t * math.cos(math.radians(10.0)), 1.0]
    return pair(E2_FACING, X)


# ---- the model ---------------------------------------------------------------------------------
def cos_min_angle(options) -> float:
    return math.cos(options.min_triangulation_angle_degrees * (math.pi / 180.0))


def unit_rays(model, K, angle_axis, pixels):
    """[n, 3]: Camera::PixelToUnitDepthRay(pixel).normalized()"""
    u = oracle.pixel_to_camera_batch(int(model), K, pixels)
    R = angle_axis_to_rotation_matrix(angle_axis)
    rays = np.zeros((len(u), 3))
    for n in range(len(u)):
        r = np.array([R[0, i] * u[n, 0] + R[1, i] * u[n, 1] + R[2, i] * u[n, 2] for i in range(3)])
        n2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2]
        rays[n] = r / math.sqrt(n2) if n2 > 0.0 else r
    return rays


def acceptable(model, ext, K, feature, X, max_sq):
    """AcceptableReprojectionError (:72-83): (accepted, margin)"""
    px, depth = oracle.project_point(int(model), ext, K, X)
    if depth < 0:
        return False, math.inf
    dx, dy = feature[0] - px[0], feature[1] - px[1]
    err = dx * dx + dy * dy
    return bool(err < max_sq), abs(err - max_sq) / max_sq


def acceptable_both(B, p, f1, f2, X, max_sq):
    """camera 1, then camera 2 (:226-238, :301-308): (accepted, the smaller margin of the tests that ran)"""
    ok, m1 = acceptable(B.model1[p], B.extrinsics1[p], B.intrinsics1[p], f1, X, max_sq)
    if not ok:
        return False, m1
    ok, m2 = acceptable(B.model2[p], B.extrinsics2[p], B.intrinsics2[p], f2, X, max_sq)
    return ok, min(m1, m2)


def triangulate(B: abi.TwoViewBatch, options):
    """Steps 1-3.  Returns (correspondence status [N], points [N, 4], margin [N], pair status [P] in {0, 1, 2},
    survivors [P])."""
    N = B.features1.shape[0]
    status = np.full(N, -1, dtype=np.int8)
    points = np.zeros((N, 4))
    margin = np.full(N, math.inf)
    pair_status = np.zeros(B.num_pairs, dtype=np.int8)
    kept = np.zeros(B.num_pairs, dtype=np.int32)
    cos_min = cos_min_angle(options)
    max_sq = options.triangulation_max_reprojection_error * options.triangulation_max_reprojection_error
    for p in range(B.num_pairs):
        c0, c1 = int(B.correspondence_ptr[p]), int(B.correspondence_ptr[p + 1])
        if c1 - c0 <= options.min_num_inlier_matches:
            pair_status[p] = 1
            continue
        r1 = unit_rays(B.model1[p], B.intrinsics1[p], B.extrinsics1[p, 3:], B.features1[c0:c1])
        r2 = unit_rays(B.model2[p], B.intrinsics2[p], B.extrinsics2[p, 3:], B.features2[c0:c1])
        origins = [B.extrinsics1[p, :3], B.extrinsics2[p, :3]]
        for i, q in enumerate(range(c0, c1)):
            a, b = r1[i], r2[i]
            dot = a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
            margin[q] = abs(dot - cos_min)
            if not dot < cos_min:
                status[q] = 1
                continue
            X = triangulate_midpoint(origins, [a, b])
            if X is None:
                status[q] = 2
                continue
            ok, m = acceptable_both(B, p, B.features1[q], B.features2[q], X, max_sq)
            margin[q] = min(margin[q], m)
            points[q] = X
            status[q] = 0 if ok else 3
        kept[p] = int((status[c0:c1] == 0).sum())
        if kept[p] < options.min_num_inlier_matches:
            pair_status[p] = 2
    return status, points, margin, pair_status, kept


def compact(B: abi.TwoViewBatch, status, points, pair_status):
    """The batch BundleAdjustTwoViews sees: the status-0 correspondences of the pairs at status 0, in order; every
    other pair with an empty range.  Returns (batch, original index [M])."""
    keep = status == 0
    keep &= np.repeat(pair_status == 0, np.diff(B.correspondence_ptr))
    idx = np.flatnonzero(keep)
    ptr = np.concatenate([[0], np.cumsum([keep[B.correspondence_ptr[p]:B.correspondence_ptr[p + 1]].sum()
                                          for p in range(B.num_pairs)])]).astype(np.int64)
    C = abi.TwoViewBatch(B.extrinsics1.copy(), B.extrinsics2.copy(), B.model1.copy(), B.model2.copy(),
                         B.intrinsics1.copy(), B.intrinsics2.copy(), B.constant_intrinsics1.copy(),
                         B.constant_intrinsics2.copy(), ptr, B.features1[idx].copy(), B.features2[idx].copy(),
                         points[idx].copy())
    return C, idx


def final_filter(C: abi.TwoViewBatch, options, pairs):
    """Steps 5-6 on an adjusted compact batch, for the pairs given.  Returns (accepted [M] bool, margin [M]); entries
    of other pairs are False / inf."""
    M = C.features1.shape[0]
    ok = np.zeros(M, dtype=bool)
    margin = np.full(M, math.inf)
    max_sq = options.final_max_reprojection_error * options.final_max_reprojection_error
    for p in pairs:
        for q in range(int(C.correspondence_ptr[p]), int(C.correspondence_ptr[p + 1])):
            ok[q], margin[q] = acceptable_both(C, p, C.features1[q], C.features2[q], C.points[q], max_sq)
    return ok, margin


def permuted(B: abi.TwoViewBatch, rng):
    """(batch with every pair's correspondences shuffled, perm) with batch.x[i] = B.x[perm[i]]."""
    perm = np.concatenate([B.correspondence_ptr[p] + rng.permutation(int(B.correspondence_ptr[p + 1] -
                                                                         B.correspondence_ptr[p]))
                           for p in range(B.num_pairs)] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    Q = B.copy()
    Q.features1, Q.features2, Q.points = B.features1[perm].copy(), B.features2[perm].copy(), B.points[perm].copy()
    return Q, perm


def verify(B: abi.TwoViewBatch, options, point_dof: int = 4, max_num_iterations: int = 200):
    """All six steps.  B is updated as tmi_ba_verify_two_views updates it.  Returns a dict with the keys of
    lib.verify_two_views (no summary) plus margin [N] (triangulation) and margin_final [N]."""
    N = B.features1.shape[0]
    status, points, margin, pair_status, kept = triangulate(B, options)
    out = {"correspondence_status": status, "pair_status": pair_status, "pair_num_verified": kept,
           "termination": np.full(B.num_pairs, -1, dtype=np.int8), "iterations": np.zeros(B.num_pairs, dtype=np.int32),
           "initial_cost": np.zeros(B.num_pairs), "final_cost": np.zeros(B.num_pairs), "margin": margin,
           "margin_final": np.full(N, math.inf)}
    written = status == 0
    B.points[written] = points[written]
    if not options.bundle_adjustment:
        return out
    C, idx = compact(B, status, points, pair_status)
    term, iters, c0, c1 = oracle.adjust_two_views(C, point_dof, max_num_iterations)
    out["termination"], out["iterations"], out["initial_cost"], out["final_cost"] = term, iters, c0, c1
    solved = pair_status == 0
    pair_status[solved & (term != 0) & (term != 1)] = 3
    good = np.flatnonzero(pair_status == 0)
    ok, mf = final_filter(C, options, good)
    for p in good:
        a, b = int(C.correspondence_ptr[p]), int(C.correspondence_ptr[p + 1])
        status[idx[a:b]] = np.where(ok[a:b], 0, 4)
        out["margin_final"][idx[a:b]] = mf[a:b]
        B.points[idx[a:b]] = C.points[a:b]
        kept[p] = int(ok[a:b].sum())
        pair_status[p] = 0 if kept[p] > options.min_num_inlier_matches else 4
        B.extrinsics2[p] = C.extrinsics2[p]
        B.intrinsics1[p, 0] = C.intrinsics1[p, 0]
        B.intrinsics2[p, 0] = C.intrinsics2[p, 0]
    return out
