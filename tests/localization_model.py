"""numpy restatement of tmi_ba_localize_views, steps 1 to 6 (include/theia_mi355_ba.h): the correspondences, the stateless
sampler, P3P, the integer costs, the replay of SampleConsensusEstimator::Estimate's loop and the final inlier mask.

Every expression of steps 2 to 6 is written in the order the device kernels evaluate it (localize_kernels.h), in IEEE
double arithmetic without contraction (Python floats for the scalars, with IEEE division and square root, numpy arrays for
the residuals), with + - * / and sqrt only, so that the model's
residuals are the device's bit for bit given the same correspondences.  ComputeMaxIterations and the confidence use
math.log / math.pow, the C library functions the engine's host side calls.

Two root paths for the quartic in cos(theta):
  "closed"   what the device does: Ferrari through a bisected root of the resolvent cubic, two Newton steps per real root
  "eigvals"  what the reference does: numpy.linalg.eigvals of the companion matrix, the real part of every root
Both give four values in ascending order.

Recorded per run: every replayed hypothesis' cost, whether it was DECISIVE (its cost within 2 of the best so far at its
turn, or it is the final model) and, over the decisive ones, the decision margin min |residual - thresh| / thresh."""
from __future__ import annotations

import math

import numpy as np

from oracle import oracle

F = float
_NAN = float("nan")


def _div(a, b):
    """IEEE a / b on Python floats (which raise where IEEE returns an infinity or a NaN)."""
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0.0:
            return _NAN
        return math.copysign(math.inf, a) * math.copysign(1.0, b)


def _sqrt(a):
    return math.sqrt(a) if a >= 0.0 else _NAN

MASK64 = (1 << 64) - 1
GAMMA = 0x9E3779B97F4A7C15


# ---- the sampler -------------------------------------------------------------------------------------------------------
def splitmix64_word(seed: int, c: int) -> int:
    """Word c of the splitmix64 stream from state `seed`: the output mix of seed + (c + 1) gamma."""
    z = (seed + (c + 1) * GAMMA) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def sample(seed: int, v: int, i: int, n: int):
    """The sample of iteration i of camera v among n correspondences: a partial Fisher-Yates on the identity."""
    a = {}
    for k in range(3):
        c = (3 * ((v << 32) + i) + k) & MASK64
        u = (float(splitmix64_word(seed, c) >> 11) + 0.5) * (1.0 / 9007199254740992.0)
        j = min(k + int(u * float(n - k)), n - 1)
        ak, aj = a.get(k, k), a.get(j, j)
        a[k], a[j] = aj, ak
    return a[0], a[1], a[2]


# ---- ComputeMaxIterations ------------------------------------------------------------------------------------------------
def compute_max_iterations(inlier_ratio: float, log_failure_prob: float, min_iterations: int, max_iterations: int) -> int:
    """sample_consensus_estimator.h:215-243 for a sample of three without the T(d,d) test."""
    if inlier_ratio == 1.0:
        return min_iterations
    log_prob = math.log(1.0 - math.pow(inlier_ratio, 3.0)) - np.finfo(np.float64).eps
    num_iterations = log_failure_prob / log_prob
    return int(max(float(min_iterations), min(num_iterations, float(max_iterations))))


# ---- P3P -----------------------------------------------------------------------------------------------------------------
def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _normalize(a):
    n = _sqrt(_dot(a, a))
    return [_div(a[0], n), _div(a[1], n), _div(a[2], n)]


def _frame(f0, f1):
    tz = _normalize(_cross(f0, f1))
    return [list(f0), _cross(tz, f0), tz]


def _matvec(T, a):
    return [_dot(T[0], a), _dot(T[1], a), _dot(T[2], a)]


def quartic_closed(B, C, D, E):
    """The device's root finder for x^4 + B x^3 + C x^2 + D x + E."""
    B2 = B * B
    p = C - F(0.375) * B2
    q = (D - F(0.5) * (B * C)) + F(0.125) * (B2 * B)
    r = ((E - F(0.25) * (B * D)) + F(0.0625) * (B2 * C)) - F(0.01171875) * (B2 * B2)
    z = F(-1.0)
    c2, c1, c0 = F(2.0) * p, p * p - F(4.0) * r, q * q
    if q == 0.0:
        if r >= 0.0:
            z = F(2.0) * _sqrt(r) - p
    else:
        hi = abs(c2) if abs(c2) > abs(c1) else abs(c1)
        hi = (hi if hi > c0 else c0) + F(1.0)
        lo = F(0.0)
        for _ in range(200):
            mid = F(0.5) * (lo + hi)
            if not (mid > lo) or not (mid < hi):
                break
            g = ((mid + c2) * mid + c1) * mid - c0
            if g > 0.0:
                hi = mid
            else:
                lo = mid
        z = hi
    if z > 0.0:
        s = _sqrt(z)
        half, qs = F(0.5) * (p + z), _div(F(0.5) * q, s)
        s1, s2, m1, m2 = s, -s, half - qs, half + qs
    else:
        disc = _sqrt(c1)
        s1, s2, m1, m2 = F(0.0), F(0.0), F(0.5) * (p - disc), F(0.5) * (p + disc)
    shift = F(0.25) * B
    x, real = [], []
    for s_, m_ in ((s1, m1), (s2, m2)):
        d_ = s_ * s_ - F(4.0) * m_
        if d_ >= 0.0:
            sq = _sqrt(d_)
            x += [F(0.5) * (-s_ - sq) - shift, F(0.5) * (-s_ + sq) - shift]
            real += [True, True]
        else:
            x += [F(-0.5) * s_ - shift, F(-0.5) * s_ - shift]
            real += [False, False]
    for k in range(4):
        if not real[k]:
            continue
        v = x[k]
        for _ in range(2):
            f = (((v + B) * v + C) * v + D) * v + E
            df = ((F(4.0) * v + F(3.0) * B) * v + F(2.0) * C) * v + D
            step = _div(f, df)
            if df != 0.0 and step == step and abs(step) < 1.0e300:
                v = v - step
        x[k] = v
    for a, b in ((0, 1), (1, 2), (0, 1), (2, 3), (1, 2), (0, 1)):
        if x[a] > x[b]:
            x[a], x[b] = x[b], x[a]
    return x


def quartic_eigvals(B, C, D, E):
    """The reference's: the real parts of the companion matrix' eigenvalues, ascending."""
    if not all(np.isfinite([B, C, D, E])):
        return [F(np.nan)] * 4
    M = np.zeros((4, 4))
    M[0] = [-B, -C, -D, -E]
    M[1, 0] = M[2, 1] = M[3, 2] = 1.0
    return [F(v) for v in sorted(np.linalg.eigvals(M).real)]


def p3p(feat, Xw, roots="closed"):
    """PoseFromThreePoints and position = -R^T t.  feat [3][2], Xw [3][3] -> list of four (R [3, 3], c [3]) or None."""
    with np.errstate(all="ignore"):
        f, X = [], []
        for i in range(3):
            fx, fy = F(feat[i][0]), F(feat[i][1])
            n = _sqrt((fx * fx + fy * fy) + F(1.0))
            f.append([fx / n, fy / n, F(1.0) / n])
            X.append([F(Xw[i][0]), F(Xw[i][1]), F(Xw[i][2])])
        w10 = [X[1][a] - X[0][a] for a in range(3)]
        w20 = [X[2][a] - X[0][a] for a in range(3)]
        cr = _cross(w10, w20)
        if _dot(cr, cr) < 1e-6:
            return None
        T = _frame(f[0], f[1])
        ip = _matvec(T, f[2])
        if ip[2] > 0.0:
            f[0], f[1] = f[1], f[0]
            X[0], X[1] = X[1], X[0]
            T = _frame(f[0], f[1])
            ip = _matvec(T, f[2])
            w10 = [X[1][a] - X[0][a] for a in range(3)]
            w20 = [X[2][a] - X[0][a] for a in range(3)]
        d = _sqrt(_dot(w10, w10))
        N0 = [_div(w10[a], d) for a in range(3)]
        N2 = _normalize(_cross(N0, w20))
        N = [N0, _cross(N2, N0), N2]
        wp = _matvec(N, w20)
        f1, f2 = _div(ip[0], ip[2]), _div(ip[1], ip[2])
        p1, p2 = wp[0], wp[1]
        cosb = _dot(f[0], f[1])
        b = _div(F(1.0), F(1.0) - cosb * cosb) - F(1.0)
        b = -_sqrt(b) if cosb < 0.0 else _sqrt(b)
        F1, F2, P1, P2, D2, Bb, f12 = f1 * f1, f2 * f2, p1 * p1, p2 * p2, d * d, b * b, f1 * f2
        two = F(2.0)
        a4 = -(P2 * P2) * ((F2 + F1) + F(1.0))
        a3 = (two * (P2 * p2) * d) * (b * (F(1.0) + F2) - f12)
        a2 = P2 * ((((((((((F2 * P2 + F1 * P2) - F2 * P1) - F2 * (D2 * Bb)) - F2 * D2) + two * (p1 * d)) +
                        two * (f12 * (p1 * (d * b)))) - P1 * F1) + two * (p1 * (F2 * d))) - D2 * Bb) - two * P1)
        a1 = (two * (p2 * d)) * (((b * P1 + f12 * P2) - F2 * (P2 * b)) - p1 * (d * b))
        a0 = (((((((F2 * (P2 * D2) - two * (f12 * (P2 * (p1 * (d * b))))) + two * (P1 * (p1 * d))) - P1 * D2) +
                  F2 * (P2 * P1)) - P1 * P1) - two * (F2 * (P2 * (p1 * d)))) + P2 * (F1 * P1)) + F2 * (P2 * (D2 * Bb))
        if a4 == 0.0:
            return None
        finder = quartic_closed if roots == "closed" else quartic_eigvals
        ct = finder(_div(a3, a4), _div(a2, a4), _div(a1, a4), _div(a0, a4))
        poses = []
        for c in ct:
            cot = _div((_div(-f1 * p1, f2) - c * p2) + d * b, (_div((-f1 * c) * p2, f2) + p1) - d)
            st = _sqrt(F(1.0) - c * c)
            sa = _sqrt(_div(F(1.0), cot * cot + F(1.0)))
            ca = _sqrt(F(1.0) - sa * sa)
            if cot < 0.0:
                ca = -ca
            kk = sa * b + ca
            cnu = [(d * ca) * kk, ((c * d) * sa) * kk, ((st * d) * sa) * kk]
            t0 = [X[0][a] + ((N[0][a] * cnu[0] + N[1][a] * cnu[1]) + N[2][a] * cnu[2]) for a in range(3)]
            Q = [[-ca, -sa * c, -sa * st], [sa, -ca * c, -ca * st], [F(0.0), -st, c]]
            A = [[(Q[i][0] * N[0][j] + Q[i][1] * N[1][j]) + Q[i][2] * N[2][j] for j in range(3)] for i in range(3)]
            R = [[(T[0][i] * A[0][j] + T[1][i] * A[1][j]) + T[2][i] * A[2][j] for j in range(3)] for i in range(3)]
            t = [-((R[i][0] * t0[0] + R[i][1] * t0[1]) + R[i][2] * t0[2]) for i in range(3)]
            pos = [-((R[0][j] * t[0] + R[1][j] * t[1]) + R[2][j] * t[2]) for j in range(3)]
            poses.append((np.array(R, dtype=np.float64), np.array(pos, dtype=np.float64)))
        return poses


def residuals(R, c, feat, X):
    """|hnormalized(R (X - c)) - feature|^2 per correspondence, in the scoring kernel's order."""
    with np.errstate(all="ignore"):
        d0, d1, d2 = X[:, 0] - c[0], X[:, 1] - c[1], X[:, 2] - c[2]
        r0 = (R[0, 0] * d0 + R[0, 1] * d1) + R[0, 2] * d2
        r1 = (R[1, 0] * d0 + R[1, 1] * d1) + R[1, 2] * d2
        r2 = (R[2, 0] * d0 + R[2, 1] * d1) + R[2, 2] * d2
        du, dv = r0 / r2 - feat[:, 0], r1 / r2 - feat[:, 1]
        return du * du + dv * dv


# ---- RANSAC ----------------------------------------------------------------------------------------------------------------
class RansacResult:
    pass


def ransac(feat, X, thresh, v=0, seed=0, samples=None, failure_probability=0.01, min_inlier_ratio=0.0,
           min_iterations=100, max_iterations=1000, roots="closed", chunk=None):
    """Steps 2 to 6 for one view.  samples: [max_iterations, 3] or None (then drawn from seed for camera v).
    chunk: None runs the sequential loop as the reference writes it; an integer evaluates the iterations chunk by chunk
    against the bound at the chunk's start and replays them, as the device does."""
    feat = np.asarray(feat, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    n = feat.shape[0]
    log_fp = math.log(failure_probability)
    bound = max_iterations
    if min_inlier_ratio > 0:
        bound = min(compute_max_iterations(min_inlier_ratio, log_fp, min_iterations, max_iterations), max_iterations)
    res = RansacResult()
    res.n = n
    res.costs = {}        # iteration -> [4] costs, or None without a model
    res.decisive = {}     # (iteration, solution) -> True
    res.margin = math.inf
    res.cost_margin = {}  # (iteration, solution) -> min |residual - thresh| / thresh
    best_cost, best = None, None
    best_key = (-1, -1)

    def evaluate(i):
        s = samples[i] if samples is not None else sample(seed, v, i, n)
        poses = p3p(feat[list(s)], X[list(s)], roots)
        if poses is None:
            return None
        out = []
        for R, c in poses:
            e = residuals(R, c, feat, X)
            with np.errstate(all="ignore"):
                m = np.abs(e - thresh) / thresh
            m = float(np.nanmin(m)) if np.isfinite(m).any() else math.inf
            out.append((int(np.count_nonzero(~(e < thresh))), R, c, m))
        return out

    def replay(i, hyp):
        nonlocal best_cost, best, best_key, bound
        res.costs[i] = None if hyp is None else [h[0] for h in hyp]
        if hyp is None:
            return
        for k, (cost, R, c, m) in enumerate(hyp):
            res.cost_margin[(i, k)] = m
            if best_cost is None or cost <= best_cost + 2:
                res.decisive[(i, k)] = True
            if best_cost is None or cost < best_cost:
                best_cost, best, best_key = cost, (R, c), (i, k)
                inliers = n - cost
                if inliers < 3:  # inlier_ratio < 3 / n
                    continue
                bound = min(compute_max_iterations(inliers / n, log_fp, min_iterations, max_iterations), bound)

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
    res.best_iteration, res.best_solution = best_key
    res.has_model = best is not None
    if best is None:
        res.inlier_mask = np.zeros(n, dtype=bool)
        res.R, res.c = None, None
    else:
        res.decisive[best_key] = True
        res.R, res.c = best
        res.inlier_mask = residuals(res.R, res.c, feat, X) < thresh
    res.num_inliers = int(np.count_nonzero(res.inlier_mask))
    ratio = res.num_inliers / n
    res.confidence = 1.0 - math.pow(1.0 - math.pow(ratio, 3.0), float(it))
    margins = [res.cost_margin[k] for k in res.decisive if k in res.cost_margin]
    res.margin = min(margins) if margins else math.inf
    return res


# ---- the call ----------------------------------------------------------------------------------------------------------------
def matrix_to_angle_axis(R):
    """Ceres' RotationMatrixToAngleAxis (through the quaternion), as rotation_kernels.h restates it."""
    import robust_rotation_model as rot
    return rot.matrix_to_angle_axis(np.asarray(R, dtype=np.float64))


def correspondences(P, c):
    """Step 1 for camera c: (observation indices ascending, features [n, 2], world points [n, 3])."""
    idx = np.nonzero(P.obs_camera == c)[0]
    g = int(P.camera_group[c])
    a, b = int(P.group_offset[g]), int(P.group_offset[g + 1])
    model = int(P.group_model[g])
    K = np.zeros(10)
    K[: b - a] = P.intrinsics[a:b]
    u = oracle.pixel_to_camera_batch(model, K, np.ascontiguousarray(P.obs_xy[idx]))
    feat = u[:, :2] / u[:, 2:3]
    Xh = P.points[P.obs_point[idx]]
    return idx, feat, Xh[:, :3] / Xh[:, 3:4]


def localize(P, thresholds, view_mask=None, samples=None, seed=0, min_num_inliers=30, roots="closed", chunk=None, **kw):
    """Steps 1 to 6 (and the status of step 7 without the adjustment) for every selected view.  Returns a dict of per-view
    arrays like lib.localize_views plus `pose` [Nc, 6], `results` {camera: RansacResult}, `margin` (the smallest decision
    margin) and `hypothesis_cost` [num_selected, max_iterations, 4]."""
    Nc = P.num_cameras
    K = kw.get("max_iterations", 1000)
    sel = [c for c in range(Nc) if view_mask is None or view_mask[c]]
    out = dict(status=np.full(Nc, -1, np.int8), num_correspondences=np.zeros(Nc, np.int32),
               num_inliers=np.zeros(Nc, np.int32), num_iterations=np.zeros(Nc, np.int32),
               best_iteration=np.full(Nc, -1, np.int32), best_solution=np.full(Nc, -1, np.int32),
               confidence=np.zeros(Nc), obs_inlier=np.zeros(P.num_observations, np.uint8), pose=np.zeros((Nc, 6)),
               hypothesis_cost=np.full((len(sel), K, 4), -1, np.int32), results={}, margin=math.inf)
    for rank, c in enumerate(sel):
        idx, feat, X = correspondences(P, c)
        n = idx.shape[0]
        out["num_correspondences"][c] = n
        if n < max(min_num_inliers, 3):
            out["status"][c] = 1
            continue
        r = ransac(feat, X, float(thresholds[c]), v=c, seed=seed, samples=None if samples is None else samples[c],
                   roots=roots, chunk=chunk, **kw)
        out["results"][c] = r
        out["margin"] = min(out["margin"], r.margin)
        for i, costs in r.costs.items():
            if costs is not None:
                out["hypothesis_cost"][rank, i] = costs
        out["num_inliers"][c] = r.num_inliers
        out["num_iterations"][c] = r.num_iterations
        out["best_iteration"][c] = r.best_iteration
        out["best_solution"][c] = r.best_solution
        out["confidence"][c] = r.confidence
        out["obs_inlier"][idx] = r.inlier_mask
        if not r.has_model:
            out["status"][c] = 2
            continue
        out["status"][c] = 3 if r.num_inliers < min_num_inliers else 0
        out["pose"][c, :3] = r.c
        out["pose"][c, 3:] = matrix_to_angle_axis(r.R)
    return out
