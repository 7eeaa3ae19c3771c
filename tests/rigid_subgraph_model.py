"""A numpy model of tmi_ba_extract_parallel_rigid_subgraph (include/theia_mi355_ba.h), i.e. of
theia::ExtractMaximallyParallelRigidSubgraph (extract_maximally_parallel_rigid_subgraph.cc:53-228) on the views that
have an edge inside the mask.

Two null-space paths:
  "eigh"  numpy.linalg.eigh of the block Laplacian L = A^T A, assembled block by block as the device assembles it;
  "svd"   the right singular vectors of the explicit 3 E x 3 V measurement matrix A of :61-84.
The search (:104-168) follows the reference statement by statement.  Every decision reports its margin:
  eigenvalues against null_tolerance x the largest diagonal entry of L  (null_max, other_min: relative values),
  row norms against 1e-10                                               (norm_below_max, norm_above_min),
  cosine distances against 1e-5                                         (cos_below_max, cos_above_min).
"""
from __future__ import annotations

import numpy as np

MAX_NORM = 1e-10          # :108
MAX_COS_DISTANCE = 1e-5   # :107


def angle_axis_to_rotation_matrix(aa):
    """ceres::AngleAxisToRotationMatrix."""
    aa = np.asarray(aa, dtype=np.float64)
    theta2 = float(aa @ aa)
    K = np.array([[0.0, -aa[2], aa[1]], [aa[2], 0.0, -aa[0]], [-aa[1], aa[0], 0.0]])
    if theta2 > np.finfo(np.float64).eps:
        theta = np.sqrt(theta2)
        w = aa / theta
        Kw = K / theta
        return np.cos(theta) * np.eye(3) + (1.0 - np.cos(theta)) * np.outer(w, w) + np.sin(theta) * Kw
    return np.eye(3) + K


def cross_matrix(d):
    return np.array([[0.0, -d[2], d[1]], [d[2], 0.0, -d[0]], [-d[1], d[0], 0.0]])


def problem_views(num_views, view1, view2, view_mask=None):
    """The views with an edge between two views of the mask, ascending, and the edges of the problem in the caller's
    order on those views.  Returns (view_of [Vp], edge_of [Ep], v1 [Ep], v2 [Ep])."""
    view1, view2 = np.asarray(view1, dtype=np.int64), np.asarray(view2, dtype=np.int64)
    inside = np.ones(len(view1), dtype=bool)
    if view_mask is not None:
        m = np.asarray(view_mask) != 0
        inside = m[view1] & m[view2]
    edge_of = np.flatnonzero(inside)
    used = np.zeros(num_views, dtype=bool)
    used[view1[edge_of]] = True
    used[view2[edge_of]] = True
    view_of = np.flatnonzero(used)
    index = -np.ones(num_views, dtype=np.int64)
    index[view_of] = np.arange(len(view_of))
    return view_of, edge_of, index[view1[edge_of]], index[view2[edge_of]]


def edge_directions(orientation, v1, position2):
    """d = R(orientation of view1)^T position_2 per edge (:66-71)."""
    return np.array([angle_axis_to_rotation_matrix(orientation[a]).T @ p for a, p in zip(v1, position2)]).reshape(-1, 3)


def measurement_matrix(num_views, v1, v2, d):
    """A of :61-84: rows 3 e .. 3 e + 2 hold -[d]x at view1 and +[d]x at view2."""
    A = np.zeros((3 * len(v1), 3 * num_views))
    for e, (a, b) in enumerate(zip(v1, v2)):
        C = cross_matrix(d[e])
        A[3 * e:3 * e + 3, 3 * a:3 * a + 3] = -C
        A[3 * e:3 * e + 3, 3 * b:3 * b + 3] = C
    return A


def laplacian(num_views, v1, v2, d):
    """L = A^T A block by block: C^T C = |d|^2 I - d d^T on both diagonal blocks, its negative between the views."""
    L = np.zeros((3 * num_views, 3 * num_views))
    for e, (a, b) in enumerate(zip(v1, v2)):
        S = cross_matrix(d[e]).T @ cross_matrix(d[e])
        L[3 * a:3 * a + 3, 3 * a:3 * a + 3] += S
        L[3 * b:3 * b + 3, 3 * b:3 * b + 3] += S
        L[3 * a:3 * a + 3, 3 * b:3 * b + 3] = -S
        L[3 * b:3 * b + 3, 3 * a:3 * a + 3] = -S
    return L


def null_space(L, A, path, null_tolerance):
    """N [n, k] orthonormal, and the relative eigenvalues on both sides of the cut."""
    n = L.shape[0]
    scale = float(np.max(np.diag(L)))
    if path == "eigh":
        w, U = np.linalg.eigh(L)
    elif path == "svd":
        _, s, Vt = np.linalg.svd(A, full_matrices=True)
        w = np.zeros(n)
        w[:len(s)] = s * s
        order = np.argsort(w, kind="stable")
        w, U = w[order], Vt.T[:, order]
    else:
        raise ValueError(path)
    null = w <= null_tolerance * scale
    k = int(null.sum())
    assert np.all(null[:k]) and not np.any(null[k:])
    margins = dict(null_max=float(np.max(np.abs(w[:k])) / scale) if k else 0.0,
                   other_min=float(w[k] / scale) if k < n else np.inf)
    return U[:, :k].copy(), scale, margins


def find_component(N, fixed):
    """FindMaximalParallelRigidComponent (:104-168) for one fixed view.  Returns (flag [V] bool, margins)."""
    V = N.shape[0] // 3
    flag = np.zeros(V, dtype=bool)
    flag[fixed] = True                                            # :112
    M = N - np.tile(N[3 * fixed:3 * fixed + 3], (V, 1))           # :114-119
    norms = np.linalg.norm(M, axis=1)                             # :123
    nz = norms > 0.0
    M[nz] = M[nz] / norms[nz, None]                               # :125 (Eigen leaves a row of norm 0 alone)
    to_match = []
    margins = dict(norm_below_max=0.0, norm_above_min=np.inf, cos_below_max=0.0, cos_above_min=np.inf)
    for i in range(V):
        if i == fixed:                                            # :132
            continue
        for x in norms[3 * i:3 * i + 3]:
            if x < MAX_NORM:
                margins["norm_below_max"] = max(margins["norm_below_max"], float(x))
            else:
                margins["norm_above_min"] = min(margins["norm_above_min"], float(x))
        if np.all(norms[3 * i:3 * i + 3] < MAX_NORM):             # :138-143
            flag[i] = True
            continue
        to_match.append(i)
    if len(to_match) > 1:                                         # :151-167, every pair a < b at once
        idx = np.array(to_match)
        B = M.reshape(V, 3, -1)[idx]                              # the 3 x k blocks of :154-159
        dist = np.max(1.0 - np.abs(np.einsum("adk,bdk->dab", B, B)), axis=0)   # :91-98: the largest of x, y, z
        a, b = np.triu_indices(len(idx), 1)
        dist = dist[a, b]
        parallel = dist < MAX_COS_DISTANCE                        # :162
        flag[idx[a[parallel]]] = True                             # :163-164
        flag[idx[b[parallel]]] = True
        if parallel.any():
            margins["cos_below_max"] = float(dist[parallel].max())
        if not parallel.all():
            margins["cos_above_min"] = float(dist[~parallel].min())
    return flag, margins


def extract(orientation, view1, view2, position2, view_mask=None, path="eigh", null_tolerance=1e-9):
    """The whole call.  Returns a dict: keep [V] uint8, component_size [V] int32, null_dimension, fixed_view (the caller's
    index), null_space [n, k], laplacian, view_of, largest_diagonal and margins (see the module's docstring)."""
    orientation = np.asarray(orientation, dtype=np.float64).reshape(-1, 3)
    position2 = np.asarray(position2, dtype=np.float64).reshape(-1, 3)
    V = orientation.shape[0]
    view_of, edge_of, v1, v2 = problem_views(V, view1, view2, view_mask)
    Vp = len(view_of)
    d = edge_directions(orientation[view_of], v1, position2[edge_of])
    L = laplacian(Vp, v1, v2, d)
    A = measurement_matrix(Vp, v1, v2, d)
    N, scale, margins = null_space(L, A, path, null_tolerance)
    flags = np.zeros((Vp, Vp), dtype=bool)
    for f in range(Vp):
        flags[f], m = find_component(N, f)
        for key, value in m.items():
            margins[key] = max(margins.get(key, 0.0), value) if key.endswith("_max") else min(margins.get(key, np.inf), value)
    sizes = flags.sum(axis=1)
    best = int(np.argmax(sizes)) if Vp else -1   # (argmax: the first of equals, as the strict > of :211)
    keep = np.zeros(V, dtype=np.uint8)
    component_size = np.zeros(V, dtype=np.int32)
    if Vp:
        keep[view_of[flags[best]]] = 1
        component_size[view_of] = sizes
    return dict(keep=keep, component_size=component_size, null_dimension=N.shape[1],
                fixed_view=int(view_of[best]) if Vp else -1, null_space=N, laplacian=L, view_of=view_of,
                largest_diagonal=scale, margins=margins)
