"""numpy restatement of tmi_ba_estimate_uncalibrated_relative_poses, steps 2 to 8 (include/theia_mi355_ba.h): the
stateless sampler, the normalised eight-point fundamental matrix, the focal lengths from it, the essential matrix'
decomposition with the cheirality vote, the integer costs, the replay of SampleConsensusEstimator::Estimate's loop and
the final inlier mask.

Every expression of steps 3 to 6 is written in the order the device kernels evaluate it (two_view_ransac_kernels.h), in
IEEE double arithmetic without contraction (Python floats for the scalars, numpy arrays for the per-correspondence
scores), with + - * / and sqrt only, so that the model's numbers are the device's bit for bit.  ComputeMaxIterations
and the confidence use math.log / math.pow, the C library functions the engine's host side calls.

Two paths:
  "closed"  what the device does: the kernel vector by elimination with full pivoting, every 3x3 SVD by the fixed
            one-sided Jacobi iteration
  "numpy"   the kernel vector of the 8x9 matrix and every 3x3 SVD through numpy.linalg.svd (the rank test stays the
            elimination's)

Per hypothesis the DECISION MARGINS are recorded (Hypothesis.margins), each relative, so that "below 1e-9" means "a
rounding error could turn the decision":
  sampson     min over the correspondences of |error - threshold| / threshold
  cheirality  min over the correspondences (and over the 8 x 2 rotations of the vote) and the two expressions
              A - B of |A - B| / (|A| + |B|)
  rank        |ratio - t| / t for ratio = |smallest pivot| / |largest pivot| and t = 8 DBL_EPSILON
  focal       for each square, |D| / (|D1| + |D2|) of its denominator D = D1 + D2 (the numerator is a product: its sign
              does not depend on rounding), and |e_x| > 0 of both epipoles
  vote_gap    best minus second-best cheirality count of the vote: an INTEGER.  It cannot be turned by rounding unless
              a cheirality margin above is small, so it does not flag a hypothesis by itself; it says where the two
              paths (whose SVD sign conventions order the four candidates differently) may pick different poses."""
from __future__ import annotations

import math

import numpy as np

from localization_model import MASK64, _div, _sqrt, splitmix64_word

F = float
EPS = 2.220446049250313e-16
RANK_THRESHOLD = 8.0 * EPS
JACOBI_SWEEPS = 10
SQRT2 = 1.4142135623730951
MARGIN = 1e-9


# ---- the sampler -------------------------------------------------------------------------------------------------------
def sample(seed: int, p: int, i: int, n: int):
    """The sample of iteration i of stream p among n correspondences: eight swaps of a partial Fisher-Yates."""
    a = {}
    for k in range(8):
        c = (8 * ((p << 32) + i) + k) & MASK64
        u = (float(splitmix64_word(seed, c) >> 11) + 0.5) * (1.0 / 9007199254740992.0)
        j = min(k + int(u * float(n - k)), n - 1)
        ak, aj = a.get(k, k), a.get(j, j)
        a[k], a[j] = aj, ak
    return tuple(a[k] for k in range(8))


def compute_max_iterations(inlier_ratio: float, log_failure_prob: float, min_iterations: int, max_iterations: int) -> int:
    """sample_consensus_estimator.h:215-243 for a sample of eight without the T(d,d) test."""
    if inlier_ratio == 1.0:
        return min_iterations
    log_prob = math.log(1.0 - math.pow(inlier_ratio, 8.0)) - np.finfo(np.float64).eps
    num_iterations = log_failure_prob / log_prob
    return int(max(float(min_iterations), min(num_iterations, float(max_iterations))))


# ---- small pieces ------------------------------------------------------------------------------------------------------
def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def normalization(x, y):
    sx, sy = x[0], y[0]
    for k in range(1, 8):
        sx = sx + x[k]
        sy = sy + y[k]
    cx, cy = sx / 8.0, sy / 8.0
    ss = 0.0
    for k in range(8):
        dx, dy = x[k] - cx, y[k] - cy
        ss = ss + (dx * dx + dy * dy)
    rms = _sqrt(ss / 8.0)
    nf = _div(SQRT2, rms)
    return nf, -(nf * cx), -(nf * cy)


def jacobi_svd(cols):
    """One-sided Jacobi on the columns `cols` ([3][3], cols[j] the j-th column).  Returns (a, v): the rotated columns
    sigma_j u_j and the columns of V, sorted by descending squared norm (stable)."""
    a = [list(c) for c in cols]
    v = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(JACOBI_SWEEPS):
        for p, q in ((0, 1), (0, 2), (1, 2)):
            ap, aq = a[p], a[q]
            alpha, beta, gamma = _dot(ap, ap), _dot(aq, aq), _dot(ap, aq)
            if gamma != 0.0:
                zeta = _div(beta - alpha, 2.0 * gamma)
                az = -zeta if zeta < 0.0 else zeta
                t = _div(1.0, az + _sqrt(1.0 + zeta * zeta))
                if zeta < 0.0:
                    t = -t
                c = _div(1.0, _sqrt(1.0 + t * t))
                s = c * t
                for r in range(3):
                    p_, q_ = ap[r], aq[r]
                    ap[r] = c * p_ - s * q_
                    aq[r] = s * p_ + c * q_
                    vp_, vq_ = v[p][r], v[q][r]
                    v[p][r] = c * vp_ - s * vq_
                    v[q][r] = s * vp_ + c * vq_
    n = [_dot(a[j], a[j]) for j in range(3)]
    for i, j in ((0, 1), (1, 2), (0, 1)):
        if n[i] < n[j]:
            n[i], n[j] = n[j], n[i]
            a[i], a[j] = a[j], a[i]
            v[i], v[j] = v[j], v[i]
    return a, v


def numpy_svd(cols):
    """The same result shape through numpy.linalg.svd."""
    A = np.array(cols, dtype=np.float64).T
    if not np.isfinite(A).all():
        nan = [F("nan")] * 3
        return [nan, nan, nan], [nan, nan, nan]
    U, S, Vt = np.linalg.svd(A)
    return [[F(U[r, j] * S[j]) for r in range(3)] for j in range(3)], [[F(Vt[j, r]) for r in range(3)] for j in range(3)]


def null_vector(r0, r1, r2):
    e = _cross(r0, r1)
    best = _dot(e, e)
    c = _cross(r0, r2)
    n = _dot(c, c)
    if n > best:
        best, e = n, c
    c = _cross(r1, r2)
    n = _dot(c, c)
    if n > best:
        e = c
    return e


def _rel(a, b):
    """|a - b| / (|a| + |b|) of an expression a - b (inf where both are 0 or something is not finite)."""
    d = abs(a) + abs(b)
    if not math.isfinite(d) or d == 0.0:
        return math.inf
    return abs(a - b) / d


def cheirality(R, p, u1, v1, u2, v2):
    """The two expressions of IsTriangulatedPointInFrontOfCameras and their relative margin."""
    d0 = (R[0] * u2 + R[3] * v2) + R[6]
    d1 = (R[1] * u2 + R[4] * v2) + R[7]
    d2 = (R[2] * u2 + R[5] * v2) + R[8]
    dir1_sq = (u1 * u1 + v1 * v1) + 1.0
    dir2_sq = (d0 * d0 + d1 * d1) + d2 * d2
    dir1_dir2 = (u1 * d0 + v1 * d1) + d2
    dir1_pos = (u1 * p[0] + v1 * p[1]) + p[2]
    dir2_pos = (d0 * p[0] + d1 * p[1]) + d2 * p[2]
    a1, b1 = dir2_sq * dir1_pos, dir1_dir2 * dir2_pos
    a2, b2 = dir1_dir2 * dir1_pos, dir1_sq * dir2_pos
    return a1 - b1, a2 - b2, min(_rel(a1, b1), _rel(a2, b2))


def eliminate(x1, y1, x2, y2):
    """Step 3 up to the kernel vector.  Returns (f [9] or None, pivot ratio, (nf1, tx1, ty1, nf2, tx2, ty2), rows)."""
    nf1, tx1, ty1 = normalization(x1, y1)
    nf2, tx2, ty2 = normalization(x2, y2)
    A = []
    for k in range(8):
        a, b = nf1 * x1[k] + tx1, nf1 * y1[k] + ty1
        c, d = nf2 * x2[k] + tx2, nf2 * y2[k] + ty2
        A.append([c * a, c * b, c, d * a, d * b, d, a, b, 1.0])
    rows = [list(r) for r in A]
    perm = list(range(9))
    norm = (nf1, tx1, ty1, nf2, tx2, ty2)
    max_pivot = min_pivot = 0.0
    for k in range(8):
        big, pr, pc = -1.0, k, k
        for r in range(k, 8):
            for c in range(k, 9):
                m = abs(A[r][c])
                if m > big:
                    big, pr, pc = m, r, c
        if not big > 0.0:
            return None, 0.0, norm, rows
        if k == 0 or big > max_pivot:
            max_pivot = big
        if k == 0 or big < min_pivot:
            min_pivot = big
        if pr != k:
            A[k], A[pr] = A[pr], A[k]
        if pc != k:
            for r in range(8):
                A[r][k], A[r][pc] = A[r][pc], A[r][k]
            perm[k], perm[pc] = perm[pc], perm[k]
        piv = A[k][k]
        for r in range(k + 1, 8):
            m = _div(A[r][k], piv)
            for c in range(k + 1, 9):
                A[r][c] = A[r][c] - m * A[k][c]
    ratio = _div(min_pivot, max_pivot)
    if not min_pivot > RANK_THRESHOLD * max_pivot:
        return None, ratio, norm, rows
    z = [0.0] * 9
    z[8] = 1.0
    for k in range(7, -1, -1):
        acc = 0.0
        for c in range(k + 1, 9):
            acc = acc + A[k][c] * z[c]
        z[k] = _div(-acc, A[k][k])
    f = [0.0] * 9
    for c in range(9):
        f[perm[c]] = z[c]
    return f, ratio, norm, rows


def unit_kernel_vector(f):
    ss, big, lead = 0.0, -1.0, 0.0
    for c in range(9):
        ss = ss + f[c] * f[c]
        m = abs(f[c])
        if m > big:
            big, lead = m, f[c]
    nrm = _sqrt(ss)
    if lead < 0.0:
        nrm = -nrm
    return [_div(f[c], nrm) for c in range(9)]


def focal_lengths(Fm, flip1=False, flip2=False):
    """Step 4 on F [3][3].  Returns (f1, f2, reason, margin): reason "" or epipole_x_zero / negative_focal_square /
    nan_focal_square.  flip1 / flip2 negate the epipoles (for the test of sign independence)."""
    e1 = null_vector(Fm[0], Fm[1], Fm[2])
    e2 = null_vector([Fm[0][0], Fm[1][0], Fm[2][0]], [Fm[0][1], Fm[1][1], Fm[2][1]], [Fm[0][2], Fm[1][2], Fm[2][2]])
    if flip1:
        e1 = [-v for v in e1]
    if flip2:
        e2 = [-v for v in e2]
    if e1[0] == 0.0 or e2[0] == 0.0:
        return None, None, "epipole_x_zero", math.inf
    r1, r2 = _sqrt(e1[0] * e1[0] + e1[1] * e1[1]), _sqrt(e2[0] * e2[0] + e2[1] * e2[1])
    cs1, sn1, cs2, sn2 = _div(e1[0], r1), _div(-e1[1], r1), _div(e2[0], r2), _div(-e2[1], r2)
    re1x, re1z = cs1 * e1[0] - sn1 * e1[1], e1[2]
    re2x, re2z = cs2 * e2[0] - sn2 * e2[1], e2[2]
    H = [[Fm[r][0] * cs1 - Fm[r][1] * sn1, Fm[r][0] * sn1 + Fm[r][1] * cs1] for r in range(2)]
    rf00, rf01 = cs2 * H[0][0] - sn2 * H[1][0], cs2 * H[0][1] - sn2 * H[1][1]
    rf10, rf11 = sn2 * H[0][0] + cs2 * H[1][0], sn2 * H[0][1] + cs2 * H[1][1]
    fa, fb, fc, fd = _div(_div(rf00, re2z), re1z), _div(rf01, re2z), _div(rf10, re1z), rf11
    d1a, d1b = ((fa * fc) * re1z) * re1z, fb * fd
    d2a, d2b = ((fa * fb) * re2z) * re2z, fc * fd
    f1_sq = _div(((-fa * fc) * re1x) * re1x, d1a + d1b)
    f2_sq = _div(((-fa * fb) * re2x) * re2x, d2a + d2b)
    margin = min(_rel(d1a, -d1b), _rel(d2a, -d2b))
    if f1_sq != f1_sq or f2_sq != f2_sq:
        return None, None, "nan_focal_square", margin
    if not f1_sq >= 0.0 or not f2_sq >= 0.0:
        return None, None, "negative_focal_square", margin
    return _sqrt(f1_sq), _sqrt(f2_sq), "", margin


class Hypothesis:
    """One sample's model: F [3][3], R [9] row-major, p [3], f1, f2 -- or none, with the reason."""

    def __init__(self):
        self.ok = False
        self.reason = ""
        self.margins = dict(sampson=math.inf, cheirality=math.inf, rank=math.inf, focal=math.inf, vote_gap=8)
        self.cost = -1

    def min_margin(self):
        m = self.margins
        return min(m["sampson"], m["cheirality"], m["rank"], m["focal"])


def hypothesis(x1, y1, x2, y2, path="closed"):
    """Steps 3 to 5 for eight correspondences (sequences of Python floats)."""
    svd = jacobi_svd if path == "closed" else numpy_svd
    h = Hypothesis()
    f, ratio, (nf1, tx1, ty1, nf2, tx2, ty2), rows = eliminate(x1, y1, x2, y2)
    h.margins["rank"] = abs(ratio - RANK_THRESHOLD) / RANK_THRESHOLD if math.isfinite(ratio) else math.inf
    if f is None:
        h.reason = "rank"
        return h
    if path != "closed":
        A = np.array(rows)
        if not np.isfinite(A).all():
            h.reason = "rank"
            return h
        f = [F(v) for v in np.linalg.svd(A)[2][8]]
    f = unit_kernel_vector(f)
    a, v = svd([[f[0], f[3], f[6]], [f[1], f[4], f[7]], [f[2], f[5], f[8]]])
    M = [[a[0][r] * v[0][c] + a[1][r] * v[1][c] for c in range(3)] for r in range(3)]
    G = [[M[r][0] * nf1, M[r][1] * nf1, (M[r][0] * tx1 + M[r][1] * ty1) + M[r][2]] for r in range(3)]
    Fm = [[nf2 * G[0][c] for c in range(3)], [nf2 * G[1][c] for c in range(3)],
          [(tx2 * G[0][c] + ty2 * G[1][c]) + G[2][c] for c in range(3)]]
    fl1, fl2, reason, fmargin = focal_lengths(Fm)
    h.margins["focal"] = fmargin
    if reason:
        h.reason = reason
        return h
    k1, k2 = [fl1, fl1, 1.0], [fl2, fl2, 1.0]
    cols = [[(k2[r] * Fm[r][c]) * k1[c] for r in range(3)] for c in range(3)]
    a, v = svd(cols)
    s0, s1 = _sqrt(_dot(a[0], a[0])), _sqrt(_dot(a[1], a[1]))
    u0 = [_div(a[0][r], s0) for r in range(3)]
    u1 = [_div(a[1][r], s1) for r in range(3)]
    u2 = _cross(u0, u1)
    v0, v1 = v[0], v[1]
    v2 = _cross(v0, v1)
    tn = _sqrt(_dot(u2, u2))
    t = [_div(u2[0], tn), _div(u2[1], tn), _div(u2[2], tn)]
    R1 = [(u0[r] * v1[c] - u1[r] * v0[c]) + u2[r] * v2[c] for r in range(3) for c in range(3)]
    R2 = [(u1[r] * v0[c] - u0[r] * v1[c]) + u2[r] * v2[c] for r in range(3) for c in range(3)]
    q1 = [(R1[c] * t[0] + R1[3 + c] * t[1]) + R1[6 + c] * t[2] for c in range(3)]
    q2 = [(R2[c] * t[0] + R2[3 + c] * t[1]) + R2[6 + c] * t[2] for c in range(3)]
    counts = [0, 0, 0, 0]
    cm = math.inf
    for k in range(8):
        p1, p2, p3, p4 = _div(x1[k], fl1), _div(y1[k], fl1), _div(x2[k], fl2), _div(y2[k], fl2)
        for base, R, q in ((0, R1, q1), (2, R2, q2)):
            ea, eb, m = cheirality(R, [-q[0], -q[1], -q[2]], p1, p2, p3, p4)
            cm = min(cm, m)
            counts[base] += 1 if (ea > 0.0 and eb > 0.0) else 0
            counts[base + 1] += 1 if (-ea > 0.0 and -eb > 0.0) else 0
    best = 0
    for k in range(1, 4):
        if counts[k] > counts[best]:
            best = k
    srt = sorted(counts, reverse=True)
    h.margins["vote_gap"] = srt[0] - srt[1]
    h.margins["cheirality"] = cm
    h.counts = counts
    h.ok = True
    h.F = Fm
    h.R = R1 if best < 2 else R2
    q = q1 if best < 2 else q2
    h.p = list(q) if (best & 1) else [-q[0], -q[1], -q[2]]
    h.f1, h.f2 = fl1, fl2
    return h


def score(h, X1, Y1, X2, Y2, thresh):
    """Step 6: (outlier mask, smallest sampson margin, smallest cheirality margin) over numpy arrays."""
    with np.errstate(all="ignore"):
        R, p, Fm = h.R, h.p, h.F
        u1, v1, u2, v2 = X1 / h.f1, Y1 / h.f1, X2 / h.f2, Y2 / h.f2
        d0 = (R[0] * u2 + R[3] * v2) + R[6]
        d1 = (R[1] * u2 + R[4] * v2) + R[7]
        d2 = (R[2] * u2 + R[5] * v2) + R[8]
        dir1_sq = (u1 * u1 + v1 * v1) + 1.0
        dir2_sq = (d0 * d0 + d1 * d1) + d2 * d2
        dir1_dir2 = (u1 * d0 + v1 * d1) + d2
        dir1_pos = (u1 * p[0] + v1 * p[1]) + p[2]
        dir2_pos = (d0 * p[0] + d1 * p[1]) + d2 * p[2]
        a1, b1 = dir2_sq * dir1_pos, dir1_dir2 * dir2_pos
        a2, b2 = dir1_dir2 * dir1_pos, dir1_sq * dir2_pos
        ea, eb = a1 - b1, a2 - b2
        l0 = (Fm[0][0] * X1 + Fm[0][1] * Y1) + Fm[0][2]
        l1 = (Fm[1][0] * X1 + Fm[1][1] * Y1) + Fm[1][2]
        l2 = (Fm[2][0] * X1 + Fm[2][1] * Y1) + Fm[2][2]
        num = (X2 * l0 + Y2 * l1) + l2
        g0 = (X2 * Fm[0][0] + Y2 * Fm[1][0]) + Fm[2][0]
        g1 = (X2 * Fm[0][1] + Y2 * Fm[1][1]) + Fm[2][1]
        den = ((g0 * g0 + g1 * g1) + l0 * l0) + l1 * l1
        err = (num * num) / den
        inlier = (ea > 0.0) & (eb > 0.0) & (err < thresh)
        ms = np.abs(err - thresh) / thresh
        ms = float(np.nanmin(ms)) if np.isfinite(ms).any() else math.inf
        mc = np.minimum(np.abs(ea) / (np.abs(a1) + np.abs(b1)), np.abs(eb) / (np.abs(a2) + np.abs(b2)))
        mc = float(np.nanmin(mc)) if np.isfinite(mc).any() else math.inf
        return ~inlier, ms, mc


# ---- RANSAC ------------------------------------------------------------------------------------------------------------
class RansacResult:
    pass


def ransac(f1, f2, thresh, p=0, seed=0, samples=None, failure_probability=0.01, min_inlier_ratio=0.0, min_iterations=10,
           max_iterations=1000, path="closed", chunk=None):
    """Steps 2 to 8 for one pair with n >= 8.  f1, f2 [n, 2] centred pixels; samples [max_iterations, 8] or None.
    chunk: None runs the sequential loop as the reference writes it; an integer evaluates the iterations chunk by chunk
    against the bound at the chunk's start and replays them, as the device does."""
    f1 = np.asarray(f1, dtype=np.float64)
    f2 = np.asarray(f2, dtype=np.float64)
    n = f1.shape[0]
    X1, Y1, X2, Y2 = (np.ascontiguousarray(a) for a in (f1[:, 0], f1[:, 1], f2[:, 0], f2[:, 1]))
    log_fp = math.log(failure_probability)
    bound = max_iterations
    if min_inlier_ratio > 0:
        bound = min(compute_max_iterations(min_inlier_ratio, log_fp, min_iterations, max_iterations), max_iterations)
    res = RansacResult()
    res.n = n
    res.hyp = {}            # iteration -> Hypothesis (with .cost)
    res.bound_changers = set()
    best_cost, best, best_it = None, None, -1

    def evaluate(i):
        s = samples[i] if samples is not None else sample(seed, p, i, n)
        s = [int(k) for k in s]
        h = hypothesis([F(X1[k]) for k in s], [F(Y1[k]) for k in s], [F(X2[k]) for k in s], [F(Y2[k]) for k in s], path)
        if h.ok:
            out, ms, mc = score(h, X1, Y1, X2, Y2, thresh)
            h.cost = int(np.count_nonzero(out))
            h.margins["sampson"] = ms
            h.margins["cheirality"] = min(h.margins["cheirality"], mc)
        return h

    def replay(i, h):
        nonlocal best_cost, best, best_it, bound
        res.hyp[i] = h
        if not h.ok:
            return
        if best_cost is None or h.cost < best_cost:
            best_cost, best, best_it = h.cost, h, i
            inliers = n - h.cost
            if inliers < 8:  # inlier_ratio < 8 / n
                return
            m = compute_max_iterations(inliers / n, log_fp, min_iterations, max_iterations)
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
        res.inlier_mask = ~score(best, X1, Y1, X2, Y2, thresh)[0]
    res.num_inliers = int(np.count_nonzero(res.inlier_mask))
    res.confidence = 1.0 - math.pow(1.0 - math.pow(res.num_inliers / n, 8.0), float(it))
    res.flagged = {i for i, h in res.hyp.items() if h.min_margin() < MARGIN}
    return res


def matrix_to_angle_axis(R):
    """Ceres' RotationMatrixToAngleAxis (through the quaternion), as rotation_kernels.h restates it."""
    import robust_rotation_model as rot
    return rot.matrix_to_angle_axis(np.asarray(R, dtype=np.float64).reshape(3, 3))


def estimate(pair_offset, feature1, feature2, thresholds, pair_mask=None, pair_stream=None, samples=None, seed=0,
             path="closed", chunk=None, **kw):
    """Steps 1 to 8 for every selected pair.  Returns a dict of per-pair arrays like
    lib.estimate_uncalibrated_relative_poses plus `results` {pair: RansacResult} and `flagged` [num_selected,
    max_iterations] bool."""
    po = np.asarray(pair_offset, dtype=np.int64)
    P = po.shape[0] - 1
    K = kw.get("max_iterations", 1000)
    f1 = np.asarray(feature1, dtype=np.float64).reshape(-1, 2)
    f2 = np.asarray(feature2, dtype=np.float64).reshape(-1, 2)
    sel = [p for p in range(P) if pair_mask is None or pair_mask[p]]
    out = dict(status=np.full(P, -1, np.int8), num_correspondences=np.zeros(P, np.int32),
               num_inliers=np.zeros(P, np.int32), num_iterations=np.zeros(P, np.int32),
               best_iteration=np.full(P, -1, np.int32), confidence=np.zeros(P), fundamental_matrix=np.zeros((P, 9)),
               focal_length1=np.zeros(P), focal_length2=np.zeros(P), rotation=np.zeros((P, 3)),
               position=np.zeros((P, 3)), corr_inlier=np.zeros(int(po[-1]), np.uint8),
               hypothesis_cost=np.full((len(sel), K), -1, np.int32), flagged=np.zeros((len(sel), K), bool), results={})
    for rank, p in enumerate(sel):
        a, b = int(po[p]), int(po[p + 1])
        n = b - a
        out["num_correspondences"][p] = n
        if n < 8:
            out["status"][p] = 1
            continue
        r = ransac(f1[a:b], f2[a:b], float(thresholds[p]), p=p if pair_stream is None else int(pair_stream[p]),
                   seed=seed, samples=None if samples is None else samples[p], path=path, chunk=chunk, **kw)
        out["results"][p] = r
        for i, h in r.hyp.items():
            out["hypothesis_cost"][rank, i] = h.cost
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
        h = r.best
        out["fundamental_matrix"][p] = np.array(h.F).T.reshape(9)  # column-major
        out["focal_length1"][p], out["focal_length2"][p] = h.f1, h.f2
        out["rotation"][p] = matrix_to_angle_axis(h.R)
        out["position"][p] = h.p
    return out


def unit_f(fm_column_major):
    """F [.., 9] column-major -> [.., 3, 3] with unit Frobenius norm and its largest-magnitude entry positive."""
    Fm = np.asarray(fm_column_major, dtype=np.float64).reshape(-1, 3, 3).transpose(0, 2, 1).copy()
    for k in range(Fm.shape[0]):
        nrm = np.linalg.norm(Fm[k])
        if nrm > 0:
            Fm[k] /= nrm
            i = np.argmax(np.abs(Fm[k]))
            if Fm[k].flat[i] < 0:
                Fm[k] = -Fm[k]
    return Fm


def model_spread(a, b):
    """MODEL_SPREAD of two outputs of estimate() (or of the device): the largest difference in F (unit Frobenius norm,
    sign fixed), the focal lengths (relative), the rotation and the position over the pairs both estimated."""
    ok = (a["status"] == 0) & (b["status"] == 0)
    if not ok.any():
        return 0.0
    d = [np.abs(unit_f(a["fundamental_matrix"][ok]) - unit_f(b["fundamental_matrix"][ok])).max()]
    for k in ("focal_length1", "focal_length2"):
        d.append((np.abs(a[k][ok] - b[k][ok]) / np.abs(a[k][ok])).max())
    for k in ("rotation", "position"):
        d.append(np.abs(a[k][ok] - b[k][ok]).max())
    return float(max(d))
