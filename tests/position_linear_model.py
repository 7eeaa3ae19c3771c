"""A numpy restatement of tmi_ba_estimate_global_positions_linear (theiasfm_amd/csrc/position_linear_kernels.h and its
host loop in pose_graph_calls.h), steps 1 to 7 of the header: the triangles in lexicographic order, the normalised
features, the baseline ratios with `sorted(...)[count // 2]` for the order statistic, the components of the surviving
triplets, the records and M = A^T A, the subspace iteration of rotation_linear_model (same start, shift, Gram-Schmidt,
Jacobi, stop rule) for one wanted pair, and the sign vote.  The factorisation and the sums are numpy's, so the device
agrees with this model to rounding amplified by the problem's conditioning, not bit for bit.

`plain` is the answer without the iteration: numpy.linalg.eigh of the same matrix."""
import math

import numpy as np

from oracle import oracle
from rotation_linear_model import BLOCK, EPS, jacobi6, mgs_pass, start_block
from track_estimator_model import angle_axis_to_rotation_matrix, triangulate_midpoint
from view_pair_filter_model import angle_axis_rotate_point

DEFAULTS = dict(max_iterations=1000, tolerance=1e-10, relative_shift=1e-9, seed=0, min_triangulation_angle_degrees=2.0)
SELECT_CAP = 1024  # lpos::kSelectCap: above it (shortest track list) the device selects in global scratch


# ---- step 1 --------------------------------------------------------------------------------------------------------------
def pair_index(view1, view2):
    return {(int(a), int(b)): e for e, (a, b) in enumerate(zip(view1, view2))}


def brute_force_triplets(num_views, view1, view2):
    """Every triangle (a < b < c) by trying all O(V^3) of them, in lexicographic order."""
    edges = pair_index(view1, view2)
    return [(a, b, c) for a in range(num_views) for b in range(a + 1, num_views) for c in range(b + 1, num_views)
            if (a, b) in edges and (a, c) in edges and (b, c) in edges]


def find_triplets(num_views, view1, view2):
    """The device's way: one work item per slot of the sorted adjacency rows, a's later neighbours looked up in b's
    row.  Returns (views [T, 3], pairs [T, 3]: the batch indices of (a, b), (a, c), (b, c))."""
    edges = pair_index(view1, view2)
    rows = [[] for _ in range(num_views)]
    for (a, b), e in edges.items():
        rows[a].append((b, e))
        rows[b].append((a, e))
    views, pairs = [], []
    for a in range(num_views):
        rows[a].sort()
    for a in range(num_views):
        for i, (b, e_ab) in enumerate(rows[a]):
            if b < a:
                continue
            in_b = dict(rows[b])
            for c, e_ac in rows[a][i + 1:]:
                if c in in_b:
                    views.append((a, b, c))
                    pairs.append((e_ab, e_ac, in_b[c]))
    return np.array(views, dtype=np.int64).reshape(-1, 3), np.array(pairs, dtype=np.int64).reshape(-1, 3)


# ---- step 2 --------------------------------------------------------------------------------------------------------------
def features(P):
    """[No, 3]: pixel_to_camera(pixel), hnormalized(), homogeneous().normalized() of every observation."""
    out = np.zeros((P.num_observations, 3))
    for c in range(P.num_cameras):
        idx = np.flatnonzero(P.obs_camera == c)
        if idx.size == 0:
            continue
        g = int(P.camera_group[c])
        K = P.intrinsics[P.group_offset[g]:P.group_offset[g + 1]]
        u = oracle.pixel_to_camera_batch(int(P.group_model[g]), K, P.obs_xy[idx])
        hx, hy = u[:, 0] / u[:, 2], u[:, 1] / u[:, 2]
        n = np.sqrt((hx * hx + hy * hy) + 1.0)
        out[idx] = np.stack([hx / n, hy / n, 1.0 / n], axis=1)
    return out


# ---- step 3 --------------------------------------------------------------------------------------------------------------
def pair_rays(rotation2, f1, f2):
    """The two directions of a two-view triangulation and their dot product."""
    R = angle_axis_to_rotation_matrix(rotation2)
    d2 = np.array([R[0, c] * f2[0] + R[1, c] * f2[1] + R[2, c] * f2[2] for c in range(3)])
    return d2, f1[0] * d2[0] + f1[1] * d2[1] + f1[2] * d2[2]


def point_depths(rotation2, position2, f1, f2, cos_min):
    """GetTriangulatedPointDepths: (depth1, depth2) or None."""
    d2, dot = pair_rays(rotation2, f1, f2)
    if not dot < cos_min:
        return None
    X = triangulate_midpoint([np.zeros(3), position2], [f1, d2])
    if X is None:
        return None
    p = X[:3] / X[3]
    q = p - position2
    return math.sqrt((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]), math.sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2])


def view_tracks(P):
    """Per view {track: observation}."""
    tracks = [dict() for _ in range(P.num_cameras)]
    for o, (c, t) in enumerate(zip(P.obs_camera, P.obs_point)):
        tracks[int(c)][int(t)] = o
    return tracks


def baselines(P, batch, views, pairs, angle_degrees, feats=None, tracks=None):
    """Per triplet: baseline [T, 3] (0 where there is none), common [T], used [T]; the number of dropped tracks; and
    angle_margin, the smallest |dot - cos_min| / cos_min over every ray pair that was tested."""
    feats = features(P) if feats is None else feats
    tracks = view_tracks(P) if tracks is None else tracks
    cos_min = math.cos(angle_degrees * (math.pi / 180.0))
    T = len(views)
    base, common, used = np.zeros((T, 3)), np.zeros(T, dtype=np.int64), np.zeros(T, dtype=np.int64)
    dropped, margin = 0, np.inf
    for t in range(T):
        a, b, c = (int(v) for v in views[t])
        e12, e13, e23 = (int(e) for e in pairs[t])
        ids = sorted(set(tracks[a]) & set(tracks[b]) & set(tracks[c]))
        common[t] = len(ids)
        r2, r3 = [], []
        for track in ids:
            f1, f2, f3 = feats[tracks[a][track]], feats[tracks[b][track]], feats[tracks[c][track]]
            depths = []
            for e, fa, fb in ((e12, f1, f2), (e13, f1, f3), (e23, f2, f3)):
                margin = min(margin, abs(pair_rays(batch.pair_rotation2[e], fa, fb)[1] - cos_min) / cos_min)
                d = point_depths(batch.pair_rotation2[e], batch.pair_position2[e], fa, fb, cos_min)
                if d is None:
                    break
                depths.append(d)
            if len(depths) < 3:
                continue
            with np.errstate(divide="ignore", invalid="ignore"):
                q2, q3 = np.float64(depths[0][0]) / depths[1][0], np.float64(depths[0][1]) / depths[2][0]
            if not (q2 > 0.0 and q3 > 0.0 and np.isfinite(q2) and np.isfinite(q3)):
                dropped += 1
                continue
            r2.append(float(q2))
            r3.append(float(q3))
        used[t] = len(r2)
        if r2:
            base[t] = (1.0, sorted(r2)[len(r2) // 2], sorted(r3)[len(r3) // 2])
    return base, common, used, dropped, margin


# ---- step 4 --------------------------------------------------------------------------------------------------------------
def components(pairs, alive):
    """label [T]: the smallest triplet of the component (triplets joined through a shared PAIR), -1 for a triplet that is
    not alive; and the chosen label: the largest component, the smallest label between equals (-1: none)."""
    T = len(pairs)
    parent = list(range(T))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    first = {}
    for t in range(T):
        if not alive[t]:
            continue
        for e in pairs[t]:
            o = first.setdefault(int(e), t)
            ra, rb = find(o), find(t)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    label = np.array([find(t) if alive[t] else -1 for t in range(T)], dtype=np.int64)
    chosen, best = -1, 0
    for lab in sorted(set(label[label >= 0].tolist())):
        size = int((label == lab).sum())
        if size > best:
            chosen, best = lab, size
    return label, chosen


# ---- step 5 --------------------------------------------------------------------------------------------------------------
def from_two_vectors(a, b):
    """Eigen's Quaterniond::FromTwoVectors(a, b).toRotationMatrix(), the device's antiparallel branch."""
    v0, v1 = a / np.linalg.norm(a), b / np.linalg.norm(b)
    c = float(v1 @ v0)
    if c < -1.0 + 1e-12:
        k = int(np.argmin(np.abs(v0)))
        axis = np.cross(v0, np.eye(3)[k])
        x, y, z = axis / np.linalg.norm(axis)
        w = 0.0
    else:
        s = math.sqrt((1.0 + c) * 2.0)
        x, y, z = np.cross(v0, v1) * (1.0 / s)
        w = s * 0.5
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    return np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, 1.0 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1.0 - (txx + tyy)]])


def triplet_blocks(batch, views, pairs, baseline, w):
    """The nine 3 x 3 blocks C[k][i] of a triplet (constraint k, slot i), linear_position_estimator.cc:365-421."""
    R0 = angle_axis_to_rotation_matrix(batch.view_rotation[views[0]])
    R1 = angle_axis_to_rotation_matrix(batch.view_rotation[views[1]])
    t01 = -(R0.T @ batch.pair_position2[pairs[0]])
    t02 = -(R0.T @ batch.pair_position2[pairs[1]])
    t12 = -(R1.T @ batch.pair_position2[pairs[2]])
    r012, r201, r120 = from_two_vectors(t12, -t01), from_two_vectors(t01, t02), from_two_vectors(-t02, -t12)
    s012, s201, s120 = baseline[0] / baseline[2], baseline[1] / baseline[0], baseline[2] / baseline[1]
    I, two = np.eye(3), -2.0 * w * np.eye(3)
    return [[(-s201 * r201 + r012.T / s012 + I) * w, (s201 * r201 - r012.T / s012 + I) * w, two],
            [(-r201.T / s201 + s120 * r120 + I) * w, two, (r201.T / s201 - s120 * r120 + I) * w],
            [two, (-s012 * r012 + r120.T / s120 + I) * w, (s012 * r012 - r120.T / s120 + I) * w]]


def system(batch, views, pairs, base):
    """Of the chosen triplets: the estimated views ascending (the first is held), the dense A [9 C, 3 (V' - 1)]."""
    est = sorted(set(int(v) for v in np.asarray(views).ravel()))
    column = {v: i - 1 for i, v in enumerate(est)}
    count = {v: 0 for v in est}
    for t in views:
        for v in t:
            count[int(v)] += 1
    n = 3 * (len(est) - 1)
    A = np.zeros((9 * len(views), n))
    for c, (t, p, b) in enumerate(zip(views, pairs, base)):
        w = 1.0 / math.sqrt(min(count[int(v)] for v in t))
        blocks = triplet_blocks(batch, [int(v) for v in t], [int(e) for e in p], b, w)
        for k in range(3):
            for i in range(3):
                col = column[int(t[i])]
                if col >= 0:
                    A[9 * c + 3 * k:9 * c + 3 * k + 3, 3 * col:3 * col + 3] = blocks[k][i]
    return est, A


# ---- step 7 --------------------------------------------------------------------------------------------------------------
def sign_votes(batch, positions, estimated):
    votes = 0
    for e in range(batch.num_pairs):
        a, b = int(batch.pair_view1[e]), int(batch.pair_view2[e])
        if not (estimated[a] and estimated[b]):
            continue
        d = positions[b] - positions[a]
        n2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        if n2 > 0.0:
            d = d / math.sqrt(n2)
        q = angle_axis_rotate_point(batch.view_rotation[a], d)
        votes += 1 if float(q @ batch.pair_position2[e]) > 0.0 else -1
    return votes


# ---- the call ------------------------------------------------------------------------------------------------------------
def prepare(P, batch, options=None):
    """Steps 1 to 5: everything up to the matrix.  Returns a dict (M is None where no triplet survives)."""
    o = dict(DEFAULTS)
    o.update(options or {})
    V = batch.num_views
    views, pairs = find_triplets(V, batch.pair_view1, batch.pair_view2)
    base, common, used, dropped, margin = baselines(P, batch, views, pairs, o["min_triangulation_angle_degrees"])
    label, chosen_label = components(pairs, used > 0)
    out = dict(options=o, triplet_view=views, triplet_pair=pairs, triplet_baseline=base, triplet_num_common=common,
               triplet_num_used=used, triplet_component=label, num_dropped=dropped, angle_margin=margin,
               num_components=len(set(label[label >= 0].tolist())), chosen=np.flatnonzero(label == chosen_label)
               if chosen_label >= 0 else np.zeros(0, dtype=np.int64), M=None, estimated=np.zeros(V, dtype=np.uint8))
    if chosen_label < 0:
        return out
    ch = out["chosen"]
    est, A = system(batch, views[ch], pairs[ch], base[ch])
    out["views"], out["M"] = est, A.T @ A
    out["estimated"][est] = 1
    return out


def _finish(batch, prep, x, out):
    V = batch.num_views
    positions = np.zeros((V, 3))
    est = prep["views"]
    positions[est[1:]] = x.reshape(-1, 3)
    votes = sign_votes(batch, positions, prep["estimated"])
    if votes < 0:
        positions = -positions
    out.update(positions=positions, sign_votes=votes, flipped=int(votes < 0))
    return out


def estimate(P, batch, options=None, prep=None):
    """The device call.  Returns prepare()'s dict with usable, order, iterations, converged, eigenvalue [2], residual,
    matrix_norm, positions [V, 3] (0 for a view that is not estimated), sign_votes, flipped, stop_margin."""
    out = dict(prepare(P, batch, options) if prep is None else prep)
    o = out["options"]
    out.update(usable=0, order=0, iterations=0, converged=0, positions=np.zeros((batch.num_views, 3)), sign_votes=0,
               flipped=0)
    M = out["M"]
    if M is None:
        return out
    n = M.shape[0]
    out["order"] = n
    norm_inf = float(np.abs(M).sum(axis=1).max())
    out["matrix_norm"] = norm_inf
    mu = o["relative_shift"] * float(np.diag(M).max())
    try:
        L = np.linalg.cholesky(M + mu * np.eye(n))
    except np.linalg.LinAlgError:
        return out
    out["usable"] = 1
    threshold = o["tolerance"] * norm_inf
    Q = start_block(n, o["seed"])
    margins = []
    while out["iterations"] < o["max_iterations"] and not out["converged"]:
        out["iterations"] += 1
        Y = np.linalg.solve(L.T, np.linalg.solve(L, Q))
        Y = mgs_pass(mgs_pass(Y))
        Z = M @ Y
        theta, W, _ = jacobi6(Y.T @ Z)
        Q, Z = Y @ W, Z @ W
        res = float(np.sqrt(((Z[:, 0] - theta[0] * Q[:, 0]) ** 2).sum()))
        out["converged"] = int(res <= threshold)
        margins.append(abs(res - threshold) / threshold)
    out.update(eigenvalue=theta[:2].copy(), residual=res, stop_margin=min(margins[-2:]))
    return _finish(batch, out, Q[:, 0], out)


def plain(P, batch, options=None, prep=None):
    """numpy.linalg.eigh of the same matrix: positions, sign_votes, flipped, eigenvalues (all, ascending).  The
    eigenvector is signed as the device signs its Ritz vectors (largest coefficient positive) before the vote."""
    out = dict(prepare(P, batch, options) if prep is None else prep)
    w, X = np.linalg.eigh(out["M"])
    x = X[:, 0]
    if x[int(np.argmax(np.abs(x)))] < 0.0:
        x = -x
    out["eigenvalues"] = w
    return _finish(batch, out, x, out)


# ---- comparisons ---------------------------------------------------------------------------------------------------------
def umeyama_errors(estimated, truth):
    """Per view |s R x + t - truth| after the similarity that best maps `estimated` onto `truth` (Umeyama 1991)."""
    x, y = np.asarray(estimated, dtype=np.float64), np.asarray(truth, dtype=np.float64)
    mx, my = x.mean(axis=0), y.mean(axis=0)
    xc, yc = x - mx, y - my
    U, S, Vt = np.linalg.svd(yc.T @ xc / len(x))
    D = np.diag([1.0, 1.0, 1.0 if np.linalg.det(U) * np.linalg.det(Vt) > 0.0 else -1.0])
    R = U @ D @ Vt
    s = float((S * np.diag(D)).sum() / (xc ** 2).sum() * len(x))
    return np.linalg.norm((s * (R @ x.T)).T + (my - s * R @ mx) - y, axis=1)


def derived_bound(c, order, tolerance, norm_inf, gap):
    """max(1e-9, c (tolerance |M|_inf + n eps |M|_inf) / (lambda_2 - lambda_1)): Davis-Kahan for one residual at the
    stop rule plus the rounding of a product with M, on a unit vector."""
    return max(1e-9, c * (tolerance * norm_inf + order * EPS * norm_inf) / gap)
