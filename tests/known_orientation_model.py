"""numpy restatement of tmi_ba_estimate_positions_known_orientation and
tmi_ba_estimate_relative_positions_known_orientation (include/theia_mi355_ba.h), written from the reference's lines:
RotateCorrespondences (estimate_absolute_pose_with_known_orientation.cc:54-73), PositionFromTwoRays
(position_from_two_rays.cc:56-83) and its Error (:106-113), RelativePoseFromTwoPointsWithKnownRotation
(relative_pose_from_two_points_with_known_rotation.cc:51-88) and its Error
(estimate_relative_pose_with_known_orientation.cc:52-58, SquaredSampsonDistance of pose/util.cc:56-68), and the replay
of SampleConsensusEstimator::Estimate's loop with either scoring.

Every expression after the rotation is written in the order the device kernels evaluate it
(known_orientation_kernels.h, ransac_core.h), in IEEE double arithmetic without contraction, with + - * / and sqrt only,
so that the "closed" path's numbers are the device's bit for bit.  The rotation calls math.sin / math.cos where the
device calls its own: estimate() therefore takes `rotated=` -- the device's rotated features -- in place of its own.

What comes from the other models: splitmix64_word, _div, _sqrt (localization_model), wave_sum -- the fixed 64-lane
shape of the MLE sum -- (homography_model), AngleAxisToRotationMatrix (track_estimator_model).  Their `sample` and
`compute_max_iterations` hard-code their own sample sizes (3, 4, 5, 8) and their RANSAC loops their own hypothesis
functions, so the sample of TWO, ComputeMaxIterations(2, ..) and the loop are written here, in the same shape.

Two paths:
  "closed"  what the device does: the position from the normal equations in closed form, the direction as a normalised
            cross product, the MLE cost as 64 lane sums combined by the xor butterfly
  "numpy"   the position through numpy.linalg.lstsq on the 4x3 system, the direction as the last right singular vector
            of the 2x3 matrix (the rank tests stay the closed path's), the MLE cost through np.sum

DECISION MARGINS per hypothesis (Hypothesis.margins), each relative:
  rank      |ratio - t| / t.  Absolute: ratio = (q / 2) / max(2, n22), t = (3 eps)^2.  Relative: ratio = smaller pivot /
            larger pivot of the two elimination steps, t = 2 eps
  residual  min over the correspondences of |r - threshold| / threshold
  replay    of cost < best under MLE: |cost - best| / max(|cost|, |best|); bitwise equal costs are a decided "not less"
A hypothesis is FLAGGED when a margin is below MARGIN (1e-9)."""
from __future__ import annotations

import math

import numpy as np

from homography_model import wave_sum
from localization_model import MASK64, _div, _sqrt, splitmix64_word
from track_estimator_model import angle_axis_to_rotation_matrix

F = float
EPS = 2.220446049250313e-16
POSITION_RANK_THRESHOLD = (3.0 * EPS) * (3.0 * EPS)
BASELINE_RANK_THRESHOLD = 2.0 * EPS
DBL_MAX = 1.7976931348623157e308
MARGIN = 1e-9
SAMPLE = 2


# ---- the sampler -------------------------------------------------------------------------------------------------------
def sample(seed: int, p: int, i: int, n: int):
    """The sample of iteration i of stream p among n correspondences: two swaps of a partial Fisher-Yates."""
    a = {}
    for k in range(SAMPLE):
        c = (SAMPLE * ((p << 32) + i) + k) & MASK64
        u = (float(splitmix64_word(seed, c) >> 11) + 0.5) * (1.0 / 9007199254740992.0)
        j = min(k + int(u * float(n - k)), n - 1)
        ak, aj = a.get(k, k), a.get(j, j)
        a[k], a[j] = aj, ak
    return tuple(a[k] for k in range(SAMPLE))


def compute_max_iterations(inlier_ratio: float, log_failure_prob: float, min_iterations: int, max_iterations: int) -> int:
    """sample_consensus_estimator.h:215-243 for a sample of two without the T(d,d) test."""
    if inlier_ratio == 1.0:
        return min_iterations
    log_prob = math.log(1.0 - math.pow(inlier_ratio, 2.0)) - np.finfo(np.float64).eps
    num_iterations = log_failure_prob / log_prob
    return int(max(float(min_iterations), min(num_iterations, float(max_iterations))))


# ---- the rotation ------------------------------------------------------------------------------------------------------
def rotate(feature, angle_axis):
    """RotateCorrespondences: hnormalized(R^T (u, v, 1)) for feature [n, 2]."""
    R = angle_axis_to_rotation_matrix(angle_axis)
    f = np.asarray(feature, dtype=np.float64).reshape(-1, 2)
    x, y = f[:, 0], f[:, 1]
    with np.errstate(all="ignore"):
        r0 = (R[0, 0] * x + R[1, 0] * y) + R[2, 0]
        r1 = (R[0, 1] * x + R[1, 1] * y) + R[2, 1]
        r2 = (R[0, 2] * x + R[1, 2] * y) + R[2, 2]
        return np.stack([r0 / r2, r1 / r2], axis=1)


class Hypothesis:
    """One sample's model: 3 doubles -- or none, with the reason."""

    def __init__(self):
        self.ok = False
        self.reason = ""
        self.model = None
        self.margins = dict(rank=math.inf, residual=math.inf, replay=math.inf)
        self.cost = -1
        self.cost_real = math.nan

    def min_margin(self):
        return min(self.margins.values())


def _rank_margin(ratio, t):
    return abs(ratio - t) / t if math.isfinite(ratio) else math.inf


# ---- the absolute problem: planes u, v, X, Y, Z ------------------------------------------------------------------------
def position_system(pts):
    """The 4x3 system of position_from_two_rays.cc:63-72 for two rows (u, v, X, Y, Z)."""
    A = np.array([[1.0, 0.0, -pts[0][0]], [0.0, 1.0, -pts[0][1]], [1.0, 0.0, -pts[1][0]], [0.0, 1.0, -pts[1][1]]])
    b = np.array([pts[0][2] - pts[0][0] * pts[0][4], pts[0][3] - pts[0][1] * pts[0][4],
                  pts[1][2] - pts[1][0] * pts[1][4], pts[1][3] - pts[1][1] * pts[1][4]])
    return A, b


def position_from_two_rays(pts, path="closed"):
    """pts: two rows (u, v, X, Y, Z) of Python floats."""
    h = Hypothesis()
    (u1, v1, X1, Y1, Z1), (u2, v2, X2, Y2, Z2) = pts
    b0, b1 = X1 - u1 * Z1, Y1 - v1 * Z1
    b2, b3 = X2 - u2 * Z2, Y2 - v2 * Z2
    du, dv = u1 - u2, v1 - v2
    q = du * du + dv * dv
    n22 = (u1 * u1 + v1 * v1) + (u2 * u2 + v2 * v2)
    big = n22 if n22 > 2.0 else 2.0
    h.margins["rank"] = _rank_margin(_div(q * 0.5, big), POSITION_RANK_THRESHOLD)
    if not q * 0.5 > POSITION_RANK_THRESHOLD * big:
        h.reason = "rank"
        return h
    if path == "closed":
        dbx, dby = b0 - b2, b1 - b3
        cz = -_div(du * dbx + dv * dby, q)
        h.model = [((b0 + u1 * cz) + (b2 + u2 * cz)) * 0.5, ((b1 + v1 * cz) + (b3 + v2 * cz)) * 0.5, cz]
    else:
        A, b = position_system(pts)
        h.model = [F(t) for t in np.linalg.lstsq(A, b, rcond=None)[0]]
    h.ok = True
    return h


def position_residuals(c, P):
    """:106-113 over the planes P [5][n]."""
    with np.errstate(all="ignore"):
        d0, d1, d2 = P[2] - c[0], P[3] - c[1], P[4] - c[2]
        du, dv = d0 / d2 - P[0], d1 / d2 - P[1]
        return du * du + dv * dv


# ---- the relative problem: planes x1, y1, x2, y2 -----------------------------------------------------------------------
def epipolar_rows(pts):
    return [[-y1 + y2, -x2 + x1, y1 * x2 - x1 * y2] for (x1, y1, x2, y2) in pts]


def baseline_pivots(e):
    """The two pivots of the elimination with full pivoting of the 2x3 rows, or None where one is not > 0."""
    p0, pr, pc = -1.0, 0, 0
    for r in range(2):
        for c in range(3):
            m = abs(e[r][c])
            if m > p0:
                p0, pr, pc = m, r, c
    if not p0 > 0.0:
        return None
    a, b = e[pr], e[1 - pr]
    mult = _div(b[pc], a[pc])
    p1 = -1.0
    for c in range(3):
        m = abs(b[c] - mult * a[c])
        if c != pc and m > p1:
            p1 = m
    if not p1 > 0.0:
        return None
    return p0, p1


def relative_position_from_two_points(pts, path="closed"):
    """pts: two rows (x1, y1, x2, y2) of Python floats."""
    h = Hypothesis()
    e = epipolar_rows(pts)
    piv = baseline_pivots(e)
    if piv is None:
        h.margins["rank"] = 1.0  # a zero pivot: ratio 0, as far from the threshold as a ratio can be on this side
        h.reason = "rank"
        return h
    mn, mx = min(piv), max(piv)
    h.margins["rank"] = _rank_margin(_div(mn, mx), BASELINE_RANK_THRESHOLD)
    if not mn > BASELINE_RANK_THRESHOLD * mx:
        h.reason = "rank"
        return h
    if path == "closed":
        c0 = e[0][1] * e[1][2] - e[0][2] * e[1][1]
        c1 = e[0][2] * e[1][0] - e[0][0] * e[1][2]
        c2 = e[0][0] * e[1][1] - e[0][1] * e[1][0]
        nrm = _sqrt((c0 * c0 + c1 * c1) + c2 * c2)
        if not nrm > 0.0 or not nrm <= DBL_MAX:
            h.reason = "norm"
            return h
        h.model = [_div(c0, nrm), _div(c1, nrm), _div(c2, nrm)]
    else:
        h.model = [F(t) for t in np.linalg.svd(np.array(e))[2][2]]
    h.ok = True
    return h


def sampson_residuals(t, P):
    """:52-58 over the planes P [4][n]."""
    with np.errstate(all="ignore"):
        l0 = t[2] * P[1] - t[1]
        l1 = t[0] - t[2] * P[0]
        l2 = t[1] * P[0] - t[0] * P[1]
        num = (P[2] * l0 + P[3] * l1) + l2
        g0 = t[1] - P[3] * t[2]
        g1 = P[2] * t[2] - t[0]
        den = ((g0 * g0 + g1 * g1) + l0 * l0) + l1 * l1
        return (num * num) / den


PROBLEMS = {
    "absolute": (position_from_two_rays, position_residuals),
    "relative": (relative_position_from_two_points, sampson_residuals),
}


def score(residual, thresh, path="closed"):
    """(inlier mask, MLE cost, smallest residual margin) of the residuals r."""
    with np.errstate(all="ignore"):
        inlier = residual < thresh
        terms = np.where(inlier, residual, thresh)
        mle = wave_sum(terms) if path == "closed" else F(np.sum(terms))
        m = np.abs(residual - thresh) / thresh
        m = float(np.nanmin(m)) if np.isfinite(m).any() else math.inf
    return inlier, mle, m


# ---- RANSAC ------------------------------------------------------------------------------------------------------------
class RansacResult:
    pass


def ransac(kind, planes, thresh, p=0, seed=0, samples=None, failure_probability=0.01, min_inlier_ratio=0.0,
           min_iterations=10, max_iterations=1000, use_mle=False, path="closed", chunk=None):
    """Steps 3 to 7 for one item with n >= 2.  planes [kPlanes][n] (the ROTATED features, then the world points);
    samples [max_iterations, 2] or None.  chunk: None runs the sequential loop as the reference writes it; an integer
    evaluates the iterations chunk by chunk against the bound at the chunk's start and replays them, as the device
    does."""
    solve, residuals = PROBLEMS[kind]
    P = [np.ascontiguousarray(a, dtype=np.float64) for a in planes]
    n = P[0].shape[0]
    log_fp = math.log(failure_probability)
    bound = max_iterations
    if min_inlier_ratio > 0:
        bound = min(compute_max_iterations(min_inlier_ratio, log_fp, min_iterations, max_iterations), max_iterations)
    res = RansacResult()
    res.n = n
    res.hyp = {}
    res.bound_changers = set()
    best_cost, best, best_it = None, None, -1

    def evaluate(i):
        s = samples[i] if samples is not None else sample(seed, p, i, n)
        h = solve([[F(a[int(k)]) for a in P] for k in s], path)
        if h.ok:
            inlier, mle, m = score(residuals(h.model, P), thresh, path)
            h.inliers = int(np.count_nonzero(inlier))
            h.cost = n - h.inliers
            h.cost_real = mle if use_mle else math.nan
            h.margins["residual"] = m
        return h

    def replay(i, h):
        nonlocal best_cost, best, best_it, bound
        res.hyp[i] = h
        if not h.ok:
            return
        c = h.cost_real if use_mle else h.cost
        if use_mle and best_cost is not None and c != best_cost:
            h.margins["replay"] = abs(c - best_cost) / max(abs(c), abs(best_cost))
        if best_cost is None or c < best_cost:
            best_cost, best, best_it = c, h, i
            if h.inliers < SAMPLE:  # inlier_ratio < 2 / n
                return
            m = compute_max_iterations(h.inliers / n, log_fp, min_iterations, max_iterations)
            if m < bound:
                bound = m
                res.bound_changers.add(i)

    it = 0
    if chunk is None:
        while it < bound:
            replay(it, evaluate(it))
            it += 1
    else:
        start = 0
        while it < bound:
            frozen = bound
            hyps = [evaluate(start + j) if start + j < frozen else None for j in range(chunk)]
            for j in range(chunk):
                if start + j >= bound:
                    break
                replay(start + j, hyps[j])
                it = start + j + 1
            start += chunk
    res.num_iterations = it
    res.best_iteration = best_it
    res.best = best
    res.has_model = best is not None
    if best is None:
        res.inlier_mask = np.zeros(n, dtype=bool)
    else:
        res.inlier_mask = score(residuals(best.model, P), thresh, path)[0]
    res.num_inliers = int(np.count_nonzero(res.inlier_mask))
    res.confidence = 1.0 - math.pow(1.0 - math.pow(res.num_inliers / n, 2.0), float(it))
    res.flagged = {i for i, h in res.hyp.items() if h.min_margin() < MARGIN}
    return res


def estimate(kind, item_offset, features, orientations, thresholds, world_point=None, item_mask=None, item_stream=None,
             samples=None, seed=0, path="closed", chunk=None, rotated=None, **kw):
    """Steps 1 to 7 for every selected item.  features / orientations: one array ([N, 2] / [P, 3]) for "absolute", two
    for "relative"; rotated: the device's rotated features (a list like `features`) to use in place of step 2.  Returns
    a dict of per-item arrays like lib.estimate_positions_known_orientation plus `results` {item: RansacResult},
    `flagged` [num_selected, max_iterations] bool and `rotated` (the list of rotated features used)."""
    po = np.asarray(item_offset, dtype=np.int64)
    N = po.shape[0] - 1
    K = kw.get("max_iterations", 1000)
    fs = [np.asarray(f, dtype=np.float64).reshape(-1, 2) for f in features]
    os_ = [np.asarray(o, dtype=np.float64).reshape(-1, 3) for o in orientations]
    X = None if world_point is None else np.asarray(world_point, dtype=np.float64).reshape(-1, 3)
    sel = [p for p in range(N) if item_mask is None or item_mask[p]]
    total = int(po[-1])
    out = dict(status=np.full(N, -1, np.int8), num_correspondences=np.zeros(N, np.int32),
               num_inliers=np.zeros(N, np.int32), num_iterations=np.zeros(N, np.int32),
               best_iteration=np.full(N, -1, np.int32), confidence=np.zeros(N), position=np.zeros((N, 3)),
               corr_inlier=np.zeros(total, np.uint8), hypothesis_cost=np.full((len(sel), K), -1, np.int32),
               hypothesis_cost_real=np.full((len(sel), K), np.nan), flagged=np.zeros((len(sel), K), bool), results={},
               rotated=[np.zeros((total, 2)) for _ in fs])
    for rank, p in enumerate(sel):
        a, b = int(po[p]), int(po[p + 1])
        n = b - a
        out["num_correspondences"][p] = n
        if n < SAMPLE:
            out["status"][p] = 1
            continue
        planes = []
        for k, f in enumerate(fs):
            r = np.asarray(rotated[k], dtype=np.float64).reshape(-1, 2)[a:b] if rotated is not None \
                else rotate(f[a:b], os_[k][p])
            out["rotated"][k][a:b] = r
            planes += [r[:, 0], r[:, 1]]
        if X is not None:
            planes += [X[a:b, 0], X[a:b, 1], X[a:b, 2]]
        r = ransac(kind, planes, float(thresholds[p]), p=p if item_stream is None else int(item_stream[p]), seed=seed,
                   samples=None if samples is None else samples[p], path=path, chunk=chunk, **kw)
        out["results"][p] = r
        for i, h in r.hyp.items():
            out["hypothesis_cost"][rank, i] = h.cost
            out["hypothesis_cost_real"][rank, i] = h.cost_real
            out["flagged"][rank, i] = i in r.flagged
        out["num_inliers"][p] = r.num_inliers
        out["num_iterations"][p] = r.num_iterations
        out["best_iteration"][p] = r.best_iteration
        out["confidence"][p] = r.confidence
        out["corr_inlier"][a:b] = r.inlier_mask
        if not r.has_model:
            out["status"][p] = 2
            continue
        out["status"][p] = 0
        out["position"][p] = r.best.model
    return out


def direction_difference(a, b):
    """1 - |cos| of the angle between two directions: ArraysEqualUpToScale's measure (test/test_utils.h:76-85)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return 1.0 - abs(float(a @ b)) / (float(np.linalg.norm(a)) * float(np.linalg.norm(b)))
