"""CPU model of the two view-pair filters (tmi_ba_filter_view_pairs_from_relative_translation and
tmi_ba_filter_view_pairs_from_orientation), numpy only.

It restates filter_view_pairs_from_relative_translation.cc:68-304 and filter_view_pairs_from_orientation.cc:55-122 with
the orders and tie rules the engine fixes where the reference's hash maps and thread pool leave them open
(include/theia_mi355_ba.h): edges in ascending edge index, the smallest view index among sources and among equal
scores, the bad weight summed in ascending iteration order.  Every arithmetic step of the ordering is one np.float64
operation, the projection three products and two sums from left to right, so the device can be held to its bits."""
from dataclasses import dataclass

import numpy as np

F = np.float64


# ---- rotations -----------------------------------------------------------------------------------------------------
def angle_axis_rotate_point(w, p):
    """ceres::AngleAxisRotatePoint with its small-angle branch (theta^2 <= DBL_EPSILON)."""
    w, p = np.asarray(w, F), np.asarray(p, F)
    theta2 = w @ w
    wxp = np.cross(w, p)
    if theta2 > np.finfo(F).eps:
        theta = np.sqrt(theta2)
        c, s = np.cos(theta), np.sin(theta)
        k = w / theta
        kxp = np.cross(k, p)
        return p * c + kxp * s + k * ((k @ p) * (F(1.0) - c))
    return p + wxp


def rotation_matrix(w):
    """ceres::AngleAxisToRotationMatrix with its first-order branch."""
    w = np.asarray(w, F)
    theta2 = w @ w
    if theta2 > np.finfo(F).eps:
        theta = np.sqrt(theta2)
        k = w / theta
        c, s = np.cos(theta), np.sin(theta)
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]], F)
        return c * np.eye(3) + s * K + (1 - c) * np.outer(k, k)
    return np.array([[1, -w[2], w[1]], [w[2], 1, -w[0]], [-w[1], w[0], 1]], F)


def rotate_translations(view_rotation, view1, position2):
    """:68-85 by Rodrigues' formula, and the spread of the MODEL: the largest difference between that and the rotation
    matrix applied as a product.  Returns (rotated [E, 3], spread)."""
    out = np.empty((len(view1), 3))
    spread = 0.0
    for e, v in enumerate(view1):
        w = -np.asarray(view_rotation[v], F)
        out[e] = angle_axis_rotate_point(w, position2[e])
        spread = max(spread, float(np.abs(out[e] - rotation_matrix(w) @ position2[e]).max()))
    return out, spread


# ---- the 1DSfM filter ------------------------------------------------------------------------------------------------
def project(t, axis):
    """[E] t . axis as ((tx ax + ty ay) + tz az), no FMA."""
    t, a = np.asarray(t, F), np.asarray(axis, F)
    return (t[:, 0] * a[0] + t[:, 1] * a[1]) + t[:, 2] * a[2]


def order_from_projections(num_views, view1, view2, p):
    """OrderTranslationsFromProjections (:114-163) with FindNextViewInOrder (:90-110).  Returns order [V] int32, -1
    for a view without edges."""
    V, E = int(num_views), len(p)
    w = np.abs(p)
    fwd = p > 0
    src = np.where(fwd, view1, view2)
    dst = np.where(fwd, view2, view1)
    in_w, out_w = np.zeros(V, F), np.zeros(V, F)
    cnt = np.zeros(V, np.int64)
    adj = [[] for _ in range(V)]
    for e in range(E):  # ascending edge index: the sequential sums
        in_w[dst[e]] += w[e]
        out_w[src[e]] += w[e]
        cnt[dst[e]] += 1
        adj[view1[e]].append((int(view2[e]), e))
        adj[view2[e]].append((int(view1[e]), e))
    remaining = np.array([len(a) > 0 for a in adj])
    order = np.full(V, -1, np.int32)
    for step in range(int(remaining.sum())):
        sources = remaining & (cnt == 0)
        if sources.any():
            win = int(np.argmax(sources))  # the smallest index
        else:
            score = np.where(remaining, (out_w + F(1.0)) / (in_w + F(1.0)), -np.inf)
            win = int(np.argmax(score))  # the first maximum: ties to the smallest index
        order[win] = step
        remaining[win] = False
        for n, e in adj[win]:
            if not remaining[n]:
                continue
            if src[e] == win:  # win -> n
                in_w[n] -= w[e]
                cnt[n] -= 1
            else:
                out_w[n] -= w[e]
    return order


@dataclass
class TranslationFilterResult:
    order: np.ndarray        # [iterations, V] int32
    contribution: np.ndarray  # [iterations, E]
    bad_weight: np.ndarray   # [E]
    removed: np.ndarray      # [E] uint8
    translation: np.ndarray  # [E, 3] the global-frame translations the ordering ran on
    spread: float            # MODEL_SPREAD of the rotation stage (0 without one)


def filter_from_relative_translation(num_views, view1, view2, position2, axes, tolerance=0.08, view_rotation=None,
                                     translation=None):
    """Steps 1-7.  translation: run from these global-frame translations instead of rotating position2."""
    view1, view2 = np.asarray(view1), np.asarray(view2)
    spread = 0.0
    if translation is not None:
        t = np.asarray(translation, F).reshape(-1, 3)
    elif view_rotation is not None:
        t, spread = rotate_translations(view_rotation, view1, np.asarray(position2, F).reshape(-1, 3))
    else:
        t = np.asarray(position2, F).reshape(-1, 3)
    axes = np.asarray(axes, F).reshape(-1, 3)
    K, E = axes.shape[0], len(view1)
    order = np.empty((K, int(num_views)), np.int32)
    contrib = np.zeros((K, E), F)
    weight = np.zeros(E, F)
    for it in range(K):
        p = project(t, axes[it])
        order[it] = order_from_projections(num_views, view1, view2, p)
        d = order[it][view2].astype(np.int64) - order[it][view1].astype(np.int64)
        bad = ((d < 0) & (p > 0)) | ((d > 0) & (p < 0))
        contrib[it] = np.where(bad, np.abs(p), F(0.0))
        weight = weight + contrib[it]  # ascending iteration order from zero
    removed = (weight > F(tolerance) * F(K)).astype(np.uint8)
    return TranslationFilterResult(order, contrib, weight, removed, t, spread)


def mean_variance(t):
    """:180-195"""
    t = np.asarray(t, F).reshape(-1, 3)
    mean = t.sum(0) / len(t)
    return mean, ((t - mean) ** 2).sum(0) / (len(t) - 1)


def draw_axes(t, num_iterations, seed):
    """:216-221 with a numpy generator: normal deviates with mean mean[k] and STANDARD DEVIATION variance[k] (the
    reference passes the variance where RandGaussian takes a standard deviation), normalised."""
    mean, var = mean_variance(t)
    a = mean + var * np.random.default_rng(seed).normal(size=(num_iterations, 3))
    return a / np.linalg.norm(a, axis=1, keepdims=True)


# ---- the orientation filter ----------------------------------------------------------------------------------------
def loop_angles(view_rotation, view1, view2, rotation2):
    """filter_view_pairs_from_orientation.cc:55-68: the angle in [0, pi] of R(-rotation_2) (R(o2) R(-o1)) as
    atan2(|skew part| / 2, (trace - 1) / 2), and the spread of the MODEL: the largest difference between that and
    arccos of the clipped (trace - 1) / 2 where the latter is well conditioned (|cos| <= 0.9), else 0 for that edge.
    Returns (angles [E], spread)."""
    R = [rotation_matrix(w) for w in view_rotation]
    out = np.empty(len(view1))
    spread = 0.0
    for e in range(len(view1)):
        L = rotation_matrix(rotation2[e]).T @ (R[view2[e]] @ R[view1[e]].T)
        s = np.array([L[2, 1] - L[1, 2], L[0, 2] - L[2, 0], L[1, 0] - L[0, 1]])
        cos_a = 0.5 * (np.trace(L) - 1.0)
        out[e] = np.arctan2(0.5 * np.sqrt(s @ s), cos_a)
        if abs(cos_a) <= 0.9:
            spread = max(spread, abs(out[e] - np.arccos(cos_a)))
    return out, spread


def filter_from_orientation(view_rotation, view1, view2, rotation2, max_degrees):
    """Returns (removed [E] uint8, angles [E], spread)."""
    angles, spread = loop_angles(view_rotation, view1, view2, rotation2)
    max_rad = F(max_degrees) * F(np.pi / 180.0)
    return (angles * angles > max_rad * max_rad).astype(np.uint8), angles, spread


# ---- the reference's test cases ------------------------------------------------------------------------------------
def line_case():
    """LineTest (filter_view_pairs_from_relative_translation_test.cc:176-204): four views on the x axis with identity
    orientation, the three path edges, and edge (0, 3) pointing along -(1, 1, 1) / sqrt(3); tolerance 0.1.
    Returns (num_views, view1, view2, position2)."""
    view1 = np.array([0, 1, 2, 0], np.int32)
    view2 = np.array([1, 2, 3, 3], np.int32)
    pos = np.array([[1.0, 0, 0], [1.0, 0, 0], [1.0, 0, 0], -np.ones(3) / np.sqrt(3.0)])
    return 4, view1, view2, pos


# (name, views, valid pairs, invalid pairs, seeds) of :206-216.  A seed gives the scene (synth.make_view_pair_batch)
# and the axes (draw_axes); the reference runs one seed of its own generator per case.  The listed seeds are seeds at
# which this model keeps at least the valid count, as the reference's test demands of its seed.
REFERENCE_CASES = (
    ("NoBadRotations", 10, 30, 0, (1, 2, 3)),
    ("FewBadRotations", 10, 30, 5, (1, 2, 3)),
    ("ManyBadRotations", 30, 100, 30, (1, 2, 3)),
)
LINE_SEEDS = (1, 2, 3)
