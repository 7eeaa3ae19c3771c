"""numpy restatement of tmi_ba_estimate_calibrated_relative_poses, steps 2 to 7 (include/theia_mi355_ba.h): the
stateless sampler, the minimal five-point solver (five_point_relative_pose.cc:212-299), the essential matrix'
decomposition with the cheirality vote over the five sampled points, the integer costs, the replay of
SampleConsensusEstimator::Estimate's loop over up to ten models per sample and the final inlier mask.

Every expression of steps 3 to 5 is written in the order the device kernels evaluate it
(two_view_calibrated_kernels.h), in IEEE double arithmetic without contraction, with + - * / and sqrt only, so that the
"closed" path's numbers are the device's bit for bit.

Two paths:
  "closed"  what the device does: every kernel and solve by elimination with full pivoting, the real eigenvalues of the
            action matrix by elementary Hessenberg reduction and the Francis double-shift QR iteration, every 3x3 SVD by
            the fixed one-sided Jacobi iteration
  "numpy"   the kernel of the 5x9 matrix through numpy.linalg.svd (brought to the elimination's gauge: the identity in
            the free rows, so that both paths pose the same polynomial system), the 10x10 solve through
            numpy.linalg.solve, the roots and their vectors through numpy.linalg.eig, every 3x3 SVD through
            numpy.linalg.svd (the rank tests stay the elimination's)

DECISION MARGINS per sample (Sample.margins), each relative:
  sampson, cheirality, vote_gap   as in two_view_ransac_model.py, the smallest over the sample's models
  rank        the smallest over the three kinds of elimination of |ratio - t| / t, ratio = |smallest pivot| / |largest
              pivot|, t = 5 eps (step 3a), 10 eps (3c), 10 eps (3e, over the nine pivots)
  root        the relative separation |a - b| / max(|a|, |b|) of the closest pair of eigenvalues of the action matrix
              (for a conjugate pair: 2 |imag| / |.|): where real / complex, or the order of two real roots, can turn
  front_gap   the smallest over the roots of |in-front count - 3.5| - 0.5, an INTEGER >= 0: like vote_gap it cannot be
              turned by rounding unless a cheirality margin is small, and flags nothing by itself
A sample is FLAGGED when sampson, cheirality or rank is below MARGIN (1e-9) or root is below ROOT_MARGIN (1e-4)."""
from __future__ import annotations

import math

import numpy as np

import two_view_ransac_model as tv
from localization_model import MASK64, _div, _sqrt, splitmix64_word

F = float
EPS = 2.220446049250313e-16
MARGIN = 1e-9
ROOT_MARGIN = 1e-4
SLOTS = 10
QR_ITERATIONS_PER_ROOT = 30
ACTION_ROWS = (0, 1, 2, 4, 5, 7)  # of the eliminated matrix (five_point_relative_pose.cc:271-275)
MINUS_ONES = ((6, 0), (7, 1), (8, 3), (9, 6))


# ---- the sampler -------------------------------------------------------------------------------------------------------
def sample(seed: int, p: int, i: int, n: int):
    """The sample of iteration i of stream p among n correspondences: five swaps of a partial Fisher-Yates."""
    a = {}
    for k in range(5):
        c = (5 * ((p << 32) + i) + k) & MASK64
        u = (float(splitmix64_word(seed, c) >> 11) + 0.5) * (1.0 / 9007199254740992.0)
        j = min(k + int(u * float(n - k)), n - 1)
        ak, aj = a.get(k, k), a.get(j, j)
        a[k], a[j] = aj, ak
    return tuple(a[k] for k in range(5))


def compute_max_iterations(inlier_ratio: float, log_failure_prob: float, min_iterations: int, max_iterations: int) -> int:
    """sample_consensus_estimator.h:215-243 for a sample of five without the T(d,d) test."""
    if inlier_ratio == 1.0:
        return min_iterations
    log_prob = math.log(1.0 - math.pow(inlier_ratio, 5.0)) - np.finfo(np.float64).eps
    num_iterations = log_failure_prob / log_prob
    return int(max(float(min_iterations), min(num_iterations, float(max_iterations))))


# ---- elimination with full pivoting -------------------------------------------------------------------------------------
def eliminate(A, nrows, npiv, ncols, steps):
    """`steps` steps of Gaussian elimination with full pivoting, in place on the list of rows A: the pivot is the entry
    of largest magnitude among rows k.. and columns k..npiv-1 (strict >, so ties go to the lowest (row, column)); the
    row swap covers all ncols columns, the column swap all rows.  Returns (perm, min_pivot, max_pivot) or None when a
    pivot is not > 0."""
    perm = list(range(npiv))
    max_pivot = min_pivot = 0.0
    for k in range(steps):
        big, pr, pc = -1.0, k, k
        for r in range(k, nrows):
            row = A[r]
            for c in range(k, npiv):
                m = abs(row[c])
                if m > big:
                    big, pr, pc = m, r, c
        if not big > 0.0:
            return None
        if k == 0 or big > max_pivot:
            max_pivot = big
        if k == 0 or big < min_pivot:
            min_pivot = big
        if pr != k:
            A[k], A[pr] = A[pr], A[k]
        if pc != k:
            for r in range(nrows):
                A[r][k], A[r][pc] = A[r][pc], A[r][k]
            perm[k], perm[pc] = perm[pc], perm[k]
        piv = A[k][k]
        rk = A[k]
        for r in range(k + 1, nrows):
            m = _div(A[r][k], piv)
            row = A[r]
            for c in range(k + 1, ncols):
                row[c] = row[c] - m * rk[c]
    return perm, min_pivot, max_pivot


def _rank_margin(min_pivot, max_pivot, t):
    ratio = _div(min_pivot, max_pivot)
    return abs(ratio - t) / t if math.isfinite(ratio) else math.inf


def epipolar_rows(x1, y1, x2, y2):
    return [[x2[k] * x1[k], y2[k] * x1[k], x1[k], x2[k] * y1[k], y2[k] * y1[k], y1[k], x2[k], y2[k], 1.0]
            for k in range(5)]


def kernel_basis(rows):
    """Step 3a.  Returns (NS [9][4] or None, rank margin, free original columns)."""
    A = [list(r) for r in rows]
    e = eliminate(A, 5, 9, 9, 5)
    if e is None:
        return None, math.inf, None
    perm, mn, mx = e
    margin = _rank_margin(mn, mx, 5.0 * EPS)
    if not mn > (5.0 * EPS) * mx:
        return None, margin, None
    NS = [[0.0] * 4 for _ in range(9)]
    for j in range(4):
        z = [0.0] * 9
        z[5 + j] = 1.0
        for k in range(4, -1, -1):
            acc = 0.0
            for c in range(k + 1, 5):
                acc = acc + A[k][c] * z[c]
            acc = acc + A[k][5 + j]
            z[k] = _div(-acc, A[k][k])
        for c in range(9):
            NS[perm[c]][j] = z[c]
    return NS, margin, perm[5:]


# ---- the polynomial expansion (five_point_relative_pose.cc:65-206) -----------------------------------------------------
def mul11(a, b):
    return [a[0] * b[0], a[0] * b[1] + a[1] * b[0], a[1] * b[1], a[0] * b[2] + a[2] * b[0], a[1] * b[2] + a[2] * b[1],
            a[2] * b[2], a[0] * b[3] + a[3] * b[0], a[1] * b[3] + a[3] * b[1], a[2] * b[3] + a[3] * b[2], a[3] * b[3]]


def mul21(a, b):
    return [a[0] * b[0],
            a[0] * b[1] + a[1] * b[0],
            a[1] * b[1] + a[2] * b[0],
            a[2] * b[1],
            a[0] * b[2] + a[3] * b[0],
            (a[1] * b[2] + a[3] * b[1]) + a[4] * b[0],
            a[2] * b[2] + a[4] * b[1],
            a[3] * b[2] + a[5] * b[0],
            a[4] * b[2] + a[5] * b[1],
            a[5] * b[2],
            a[0] * b[3] + a[6] * b[0],
            (a[1] * b[3] + a[6] * b[1]) + a[7] * b[0],
            a[2] * b[3] + a[7] * b[1],
            (a[3] * b[3] + a[6] * b[2]) + a[8] * b[0],
            (a[4] * b[3] + a[7] * b[2]) + a[8] * b[1],
            a[5] * b[3] + a[8] * b[2],
            a[6] * b[3] + a[9] * b[0],
            a[7] * b[3] + a[9] * b[1],
            a[8] * b[3] + a[9] * b[2],
            a[9] * b[3]]


def constraint_matrix(NS):
    """Step 3b: [10][20].  ns[i][j] is row i + 3 j of NS: entry (i, j) of E over the basis (:256-260)."""
    ns = [[NS[i + 3 * j] for j in range(3)] for i in range(3)]
    eet = [[None] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            m0, m1, m2 = mul11(ns[i][0], ns[j][0]), mul11(ns[i][1], ns[j][1]), mul11(ns[i][2], ns[j][2])
            eet[i][j] = [2.0 * ((m0[q] + m1[q]) + m2[q]) for q in range(10)]
    trace = [(eet[0][0][q] + eet[1][1][q]) + eet[2][2][q] for q in range(10)]
    C = []
    for i in range(3):
        for j in range(3):
            a, b, c = mul21(eet[i][0], ns[0][j]), mul21(eet[i][1], ns[1][j]), mul21(eet[i][2], ns[2][j])
            d = mul21(trace, ns[i][j])
            C.append([((a[q] + b[q]) + c[q]) - 0.5 * d[q] for q in range(20)])

    def minor(a, b, c, d, e):
        p, q = mul11(a, b), mul11(c, d)
        return mul21([p[k] - q[k] for k in range(10)], e)
    d0 = minor(ns[0][1], ns[1][2], ns[0][2], ns[1][1], ns[2][0])
    d1 = minor(ns[0][2], ns[1][0], ns[0][0], ns[1][2], ns[2][1])
    d2 = minor(ns[0][0], ns[1][1], ns[0][1], ns[1][0], ns[2][2])
    C.append([(d0[q] + d1[q]) + d2[q] for q in range(20)])
    return C


def solve_constraints(C):
    """Step 3c: X [10][10] with C[:, :10] X = C[:, 10:], row v the variable v, or None; the rank margin."""
    A = [list(r) for r in C]
    e = eliminate(A, 10, 10, 20, 10)
    if e is None:
        return None, math.inf
    perm, mn, mx = e
    margin = _rank_margin(mn, mx, 10.0 * EPS)
    if not mn > (10.0 * EPS) * mx:
        return None, margin
    for k in range(9, -1, -1):
        for j in range(10, 20):
            acc = 0.0
            for c in range(k + 1, 10):
                acc = acc + A[k][c] * A[c][j]
            A[k][j] = _div(A[k][j] - acc, A[k][k])
    X = [None] * 10
    for k in range(10):
        X[perm[k]] = A[k][10:]
    return X, margin


def action_matrix(X):
    A = [list(X[v]) for v in ACTION_ROWS] + [[0.0] * 10 for _ in range(4)]
    for r, c in MINUS_ONES:
        A[r][c] = -1.0
    return A


# ---- the real eigenvalues: elementary Hessenberg reduction, then Francis double-shift QR (EISPACK elmhes, hqr) ----------
def _sign(a, b):
    a = -a if a < 0.0 else a
    return a if b >= 0.0 else -a


def hessenberg(a):
    n = 10
    for m in range(1, n - 1):
        x, i = 0.0, m
        for j in range(m, n):
            if abs(a[j][m - 1]) > abs(x):
                x, i = a[j][m - 1], j
        if i != m:
            for j in range(m - 1, n):
                a[i][j], a[m][j] = a[m][j], a[i][j]
            for j in range(n):
                a[j][i], a[j][m] = a[j][m], a[j][i]
        if x != 0.0:
            for i in range(m + 1, n):
                y = a[i][m - 1]
                if y != 0.0:
                    y = _div(y, x)
                    a[i][m - 1] = y
                    for j in range(m, n):
                        a[i][j] = a[i][j] - y * a[m][j]
                    for j in range(n):
                        a[j][m] = a[j][m] + y * a[j][i]
    for i in range(2, n):
        for j in range(i - 1):
            a[i][j] = 0.0


def hqr(a):
    """The eigenvalues of the upper Hessenberg a [10][10] (destroyed): (wr, wi, real) with real[k] True for a 1x1 block
    or a member of a 2x2 block of non-negative discriminant; None after QR_ITERATIONS_PER_ROOT sweeps on one block."""
    n = 10
    wr, wi, real = [0.0] * n, [0.0] * n, [False] * n
    anorm = 0.0
    for i in range(n):
        for j in range(max(i - 1, 0), n):
            anorm = anorm + abs(a[i][j])
    nn, t = n - 1, 0.0
    while nn >= 0:
        its = 0
        while True:
            l = nn
            while l >= 1:
                s = abs(a[l - 1][l - 1]) + abs(a[l][l])
                if s == 0.0:
                    s = anorm
                if abs(a[l][l - 1]) + s == s:
                    a[l][l - 1] = 0.0
                    break
                l -= 1
            x = a[nn][nn]
            if l == nn:
                wr[nn], wi[nn], real[nn] = x + t, 0.0, True
                nn -= 1
                break
            y = a[nn - 1][nn - 1]
            w = a[nn][nn - 1] * a[nn - 1][nn]
            if l == nn - 1:
                p = 0.5 * (y - x)
                q = p * p + w
                z = _sqrt(-q if q < 0.0 else q)
                x = x + t
                if q >= 0.0:
                    z = p + _sign(z, p)
                    wr[nn - 1] = wr[nn] = x + z
                    if z != 0.0:
                        wr[nn] = x - _div(w, z)
                    wi[nn - 1] = wi[nn] = 0.0
                    real[nn - 1] = real[nn] = True
                else:
                    wr[nn - 1] = wr[nn] = x + p
                    wi[nn - 1], wi[nn] = z, -z
                nn -= 2
                break
            if its == QR_ITERATIONS_PER_ROOT:
                return None
            if its == 10 or its == 20:
                t = t + x
                for i in range(nn + 1):
                    a[i][i] = a[i][i] - x
                s = abs(a[nn][nn - 1]) + abs(a[nn - 1][nn - 2])
                y = x = 0.75 * s
                w = -0.4375 * (s * s)
            its += 1
            m = nn - 2
            while True:
                z = a[m][m]
                r = x - z
                s = y - z
                p = _div(r * s - w, a[m + 1][m]) + a[m][m + 1]
                q = ((a[m + 1][m + 1] - z) - r) - s
                r = a[m + 2][m + 1]
                s = (abs(p) + abs(q)) + abs(r)
                p, q, r = _div(p, s), _div(q, s), _div(r, s)
                if m == l:
                    break
                u = abs(a[m][m - 1]) * (abs(q) + abs(r))
                v = abs(p) * ((abs(a[m - 1][m - 1]) + abs(z)) + abs(a[m + 1][m + 1]))
                if u + v == v:
                    break
                m -= 1
            for i in range(m + 2, nn + 1):
                a[i][i - 2] = 0.0
                if i != m + 2:
                    a[i][i - 3] = 0.0
            for k in range(m, nn):
                if k != m:
                    p = a[k][k - 1]
                    q = a[k + 1][k - 1]
                    r = a[k + 2][k - 1] if k != nn - 1 else 0.0
                    x = (abs(p) + abs(q)) + abs(r)
                    if x == 0.0:
                        continue
                    p, q, r = _div(p, x), _div(q, x), _div(r, x)
                s = _sign(_sqrt((p * p + q * q) + r * r), p)
                if s == 0.0:
                    continue
                if k == m:
                    if l != m:
                        a[k][k - 1] = -a[k][k - 1]
                else:
                    a[k][k - 1] = -(s * x)
                p = p + s
                x, y, z = _div(p, s), _div(q, s), _div(r, s)
                q, r = _div(q, p), _div(r, p)
                for j in range(k, nn + 1):
                    p = a[k][j] + q * a[k + 1][j]
                    if k != nn - 1:
                        p = p + r * a[k + 2][j]
                        a[k + 2][j] = a[k + 2][j] - p * z
                    a[k + 1][j] = a[k + 1][j] - p * y
                    a[k][j] = a[k][j] - p * x
                mmin = nn if nn < k + 3 else k + 3
                for i in range(l, mmin + 1):
                    p = x * a[i][k] + y * a[i][k + 1]
                    if k != nn - 1:
                        p = p + z * a[i][k + 2]
                        a[i][k + 2] = a[i][k + 2] - p * r
                    a[i][k + 1] = a[i][k + 1] - p * q
                    a[i][k] = a[i][k] - p
    return wr, wi, real


def root_margin(wr, wi):
    m = math.inf
    for i in range(10):
        for j in range(i + 1, 10):
            d = math.hypot(wr[i] - wr[j], wi[i] - wi[j])
            s = max(math.hypot(wr[i], wi[i]), math.hypot(wr[j], wi[j]))
            if math.isfinite(d) and s > 0.0:
                m = min(m, d / s)
    return m


def sorted_real_roots(wr, real):
    """The real roots in ascending order: an insertion sort with a strict > (equal roots keep their order)."""
    out = []
    for k in range(10):
        if real[k]:
            v = wr[k]
            q = len(out)
            out.append(v)
            while q > 0 and out[q - 1] > v:
                out[q] = out[q - 1]
                q -= 1
            out[q] = v
    return out


def root_vector_tail(A, lam):
    """Step 3e: the last four entries of the null vector of A - lam I (nine elimination steps, the tenth permuted
    entry 1), or None; the rank margin."""
    W = [list(r) for r in A]
    for k in range(10):
        W[k][k] = W[k][k] - lam
    e = eliminate(W, 10, 10, 10, 9)
    if e is None:
        return None, math.inf
    perm, mn, mx = e
    margin = _rank_margin(mn, mx, 10.0 * EPS)
    if not mn > (10.0 * EPS) * mx:
        return None, margin
    z = [0.0] * 10
    z[9] = 1.0
    for k in range(8, -1, -1):
        acc = 0.0
        for c in range(k + 1, 10):
            acc = acc + W[k][c] * z[c]
        z[k] = _div(-acc, W[k][k])
    v = [0.0] * 10
    for c in range(10):
        v[perm[c]] = z[c]
    return v[6:], margin


def essential_from_tail(NS, t):
    e = [((NS[r][0] * t[0] + NS[r][1] * t[1]) + NS[r][2] * t[2]) + NS[r][3] * t[3] for r in range(9)]
    e = tv.unit_kernel_vector(e)
    return [[e[r + 3 * c] for c in range(3)] for r in range(3)]  # e is column-major (:293-294)


# ---- the decomposition and the vote (two_view_ransac_kernels.h, with focal lengths 1) ----------------------------------
def pose_from_essential(E, x1, y1, x2, y2, svd):
    """Returns (R [9] row-major, p [3], best count, counts, smallest cheirality margin)."""
    cols = [[E[r][c] for r in range(3)] for c in range(3)]
    a, v = svd(cols)
    s0, s1 = _sqrt(tv._dot(a[0], a[0])), _sqrt(tv._dot(a[1], a[1]))
    u0 = [_div(a[0][r], s0) for r in range(3)]
    u1 = [_div(a[1][r], s1) for r in range(3)]
    u2 = tv._cross(u0, u1)
    v0, v1 = v[0], v[1]
    v2 = tv._cross(v0, v1)
    tn = _sqrt(tv._dot(u2, u2))
    t = [_div(u2[0], tn), _div(u2[1], tn), _div(u2[2], tn)]
    R1 = [(u0[r] * v1[c] - u1[r] * v0[c]) + u2[r] * v2[c] for r in range(3) for c in range(3)]
    R2 = [(u1[r] * v0[c] - u0[r] * v1[c]) + u2[r] * v2[c] for r in range(3) for c in range(3)]
    q1 = [(R1[c] * t[0] + R1[3 + c] * t[1]) + R1[6 + c] * t[2] for c in range(3)]
    q2 = [(R2[c] * t[0] + R2[3 + c] * t[1]) + R2[6 + c] * t[2] for c in range(3)]
    counts = [0, 0, 0, 0]
    cm = math.inf
    for k in range(5):
        for base, R, q in ((0, R1, q1), (2, R2, q2)):
            ea, eb, m = tv.cheirality(R, [-q[0], -q[1], -q[2]], x1[k], y1[k], x2[k], y2[k])
            cm = min(cm, m)
            counts[base] += 1 if (ea > 0.0 and eb > 0.0) else 0
            counts[base + 1] += 1 if (-ea > 0.0 and -eb > 0.0) else 0
    best = 0
    for k in range(1, 4):
        if counts[k] > counts[best]:
            best = k
    R = R1 if best < 2 else R2
    q = q1 if best < 2 else q2
    p = list(q) if (best & 1) else [-q[0], -q[1], -q[2]]
    return R, p, counts[best], counts, cm


class Model:
    """One solution of a sample: E [3][3] (unit norm), R [9] row-major, p [3]; the fields tv.score reads."""
    f1 = f2 = 1.0
    cost = -1


class Sample:
    def __init__(self):
        self.models = []
        self.reason = ""
        self.num_real_roots = 0
        self.margins = dict(sampson=math.inf, cheirality=math.inf, rank=math.inf, root=math.inf, vote_gap=5, front_gap=5)

    @property
    def ok(self):
        return bool(self.models)

    def flagged(self):
        m = self.margins
        return min(m["sampson"], m["cheirality"], m["rank"]) < MARGIN or m["root"] < ROOT_MARGIN


def _numpy_kernel(rows, free):
    A = np.array(rows)
    V = np.linalg.svd(A)[2][5:9].T  # [9, 4]
    B = V @ np.linalg.inv(V[list(free), :])
    return [[F(B[r, j]) for j in range(4)] for r in range(9)]


def five_point(x1, y1, x2, y2, path="closed"):
    """Steps 3 and 4 for five correspondences (sequences of Python floats): a Sample."""
    svd = tv.jacobi_svd if path == "closed" else tv.numpy_svd
    h = Sample()
    rows = epipolar_rows(x1, y1, x2, y2)
    NS, margin, free = kernel_basis(rows)
    h.margins["rank"] = margin
    if NS is None:
        h.reason = "rank5"
        return h
    if path != "closed":
        if not np.isfinite(np.array(rows)).all():
            h.reason = "rank5"
            return h
        NS = _numpy_kernel(rows, free)
    C = constraint_matrix(NS)
    X, margin = solve_constraints(C)
    h.margins["rank"] = min(h.margins["rank"], margin)
    if X is None:
        h.reason = "rank10"
        return h
    if path != "closed":
        Cn = np.array(C)
        if not np.isfinite(Cn).all():
            h.reason = "rank10"
            return h
        Xn = np.linalg.solve(Cn[:, :10], Cn[:, 10:])
        X = [[F(v) for v in Xn[r]] for r in range(10)]
    A = action_matrix(X)
    if path == "closed":
        H = [list(r) for r in A]
        hessenberg(H)
        eig = hqr(H)
        if eig is None:
            h.reason = "qr"
            return h
        wr, wi, real = eig
        h.margins["root"] = root_margin(wr, wi)
        roots = sorted_real_roots(wr, real)
        tails = []
        for lam in roots:
            t, margin = root_vector_tail(A, lam)
            h.margins["rank"] = min(h.margins["rank"], margin)
            tails.append(t)
    else:
        An = np.array(A)
        if not np.isfinite(An).all():
            h.reason = "qr"
            return h
        w, V = np.linalg.eig(An)
        h.margins["root"] = root_margin([F(v.real) for v in w], [F(v.imag) for v in w])
        order = sorted((k for k in range(10) if w[k].imag == 0.0), key=lambda k: w[k].real)
        roots = [F(w[k].real) for k in order]
        tails = [[F(v) for v in V[6:, k].real] for k in order]
    h.num_real_roots = len(roots)
    h.eigenvalues = roots
    for t in tails:
        if t is None:
            continue
        E = essential_from_tail(NS, t)
        R, p, front, counts, cm = pose_from_essential(E, x1, y1, x2, y2, svd)
        h.margins["cheirality"] = min(h.margins["cheirality"], cm)
        srt = sorted(counts, reverse=True)
        h.margins["vote_gap"] = min(h.margins["vote_gap"], srt[0] - srt[1])
        h.margins["front_gap"] = min(h.margins["front_gap"], front - 4 if front >= 4 else 3 - front)
        if front >= 4:
            m = Model()
            m.F, m.R, m.p = E, R, p
            h.models.append(m)
    if not h.models:
        h.reason = "no_real_root" if not roots else "cheirality"
    return h


def sampson(E, x1, y1, x2, y2):
    """SquaredSampsonDistance (pose/util.cc:56-68) in the device's order."""
    l0 = (E[0][0] * x1 + E[0][1] * y1) + E[0][2]
    l1 = (E[1][0] * x1 + E[1][1] * y1) + E[1][2]
    l2 = (E[2][0] * x1 + E[2][1] * y1) + E[2][2]
    num = (x2 * l0 + y2 * l1) + l2
    g0 = (x2 * E[0][0] + y2 * E[1][0]) + E[2][0]
    g1 = (x2 * E[0][1] + y2 * E[1][1]) + E[2][1]
    return (num * num) / (((g0 * g0 + g1 * g1) + l0 * l0) + l1 * l1)


# ---- RANSAC ------------------------------------------------------------------------------------------------------------
class RansacResult:
    pass


def ransac(f1, f2, thresh, p=0, seed=0, samples=None, failure_probability=0.01, min_inlier_ratio=0.0, min_iterations=10,
           max_iterations=1000, path="closed", chunk=None):
    """Steps 2 to 7 for one pair with n >= 5.  f1, f2 [n, 2] normalised; samples [max_iterations, 5] or None.  chunk as
    in two_view_ransac_model.ransac."""
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
    res.hyp = {}            # iteration -> Sample (its models with .cost)
    res.bound_changers = set()
    best_cost, best, best_it, best_sol = None, None, -1, -1

    def evaluate(i):
        s = samples[i] if samples is not None else sample(seed, p, i, n)
        s = [int(k) for k in s]
        h = five_point([F(X1[k]) for k in s], [F(Y1[k]) for k in s], [F(X2[k]) for k in s], [F(Y2[k]) for k in s], path)
        for m in h.models:
            out, ms, mc = tv.score(m, X1, Y1, X2, Y2, thresh)
            m.cost = int(np.count_nonzero(out))
            h.margins["sampson"] = min(h.margins["sampson"], ms)
            h.margins["cheirality"] = min(h.margins["cheirality"], mc)
        return h

    def replay(i, h):
        nonlocal best_cost, best, best_it, best_sol, bound
        res.hyp[i] = h
        for k, m in enumerate(h.models):
            if best_cost is None or m.cost < best_cost:
                best_cost, best, best_it, best_sol = m.cost, m, i, k
                inliers = n - m.cost
                if inliers < 5:  # inlier_ratio < 5 / n
                    continue
                b = compute_max_iterations(inliers / n, log_fp, min_iterations, max_iterations)
                if b < bound:
                    bound = b
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
    res.best_iteration, res.best_solution = best_it, best_sol
    res.best = best
    res.has_model = best is not None
    if best is None:
        res.inlier_mask = np.zeros(n, dtype=bool)
    else:
        res.inlier_mask = ~tv.score(best, X1, Y1, X2, Y2, thresh)[0]
    res.num_inliers = int(np.count_nonzero(res.inlier_mask))
    res.confidence = 1.0 - math.pow(1.0 - math.pow(res.num_inliers / n, 5.0), float(it))
    res.flagged = {i for i, h in res.hyp.items() if h.flagged()}
    return res


def estimate(pair_offset, feature1, feature2, thresholds, pair_mask=None, pair_stream=None, samples=None, seed=0,
             path="closed", chunk=None, **kw):
    """Steps 1 to 7 for every selected pair.  Returns a dict of per-pair arrays like
    lib.estimate_calibrated_relative_poses plus `results` {pair: RansacResult} and `flagged` [num_selected,
    max_iterations] bool."""
    po = np.asarray(pair_offset, dtype=np.int64)
    P = po.shape[0] - 1
    K = kw.get("max_iterations", 1000)
    f1 = np.asarray(feature1, dtype=np.float64).reshape(-1, 2)
    f2 = np.asarray(feature2, dtype=np.float64).reshape(-1, 2)
    sel = [p for p in range(P) if pair_mask is None or pair_mask[p]]
    out = dict(status=np.full(P, -1, np.int8), num_correspondences=np.zeros(P, np.int32),
               num_inliers=np.zeros(P, np.int32), num_iterations=np.zeros(P, np.int32),
               best_iteration=np.full(P, -1, np.int32), best_solution=np.full(P, -1, np.int32), confidence=np.zeros(P),
               essential_matrix=np.zeros((P, 9)), rotation=np.zeros((P, 3)), position=np.zeros((P, 3)),
               corr_inlier=np.zeros(int(po[-1]), np.uint8),
               hypothesis_cost=np.full((len(sel), K, SLOTS), -1, np.int32), flagged=np.zeros((len(sel), K), bool),
               results={})
    for rank, p in enumerate(sel):
        a, b = int(po[p]), int(po[p + 1])
        n = b - a
        out["num_correspondences"][p] = n
        if n < 5:
            out["status"][p] = 1
            continue
        r = ransac(f1[a:b], f2[a:b], float(thresholds[p]), p=p if pair_stream is None else int(pair_stream[p]),
                   seed=seed, samples=None if samples is None else samples[p], path=path, chunk=chunk, **kw)
        out["results"][p] = r
        for i, h in r.hyp.items():
            for k, m in enumerate(h.models):
                out["hypothesis_cost"][rank, i, k] = m.cost
            out["flagged"][rank, i] = i in r.flagged
        out["num_inliers"][p] = r.num_inliers
        out["num_iterations"][p] = r.num_iterations
        out["best_iteration"][p] = r.best_iteration
        out["best_solution"][p] = r.best_solution
        out["confidence"][p] = r.confidence
        out["corr_inlier"][a:b] = r.inlier_mask
        if not r.has_model:
            out["status"][p] = 2
            continue
        out["status"][p] = 0
        h = r.best
        out["essential_matrix"][p] = np.array(h.F).T.reshape(9)  # column-major
        out["rotation"][p] = tv.matrix_to_angle_axis(h.R)
        out["position"][p] = h.p
    return out


def model_spread(a, b):
    """MODEL_SPREAD of two outputs of estimate() (or of the device): the largest difference in E (unit Frobenius norm,
    sign fixed), the rotation and the position over the pairs both estimated."""
    ok = (a["status"] == 0) & (b["status"] == 0)
    if not ok.any():
        return 0.0
    d = [np.abs(tv.unit_f(a["essential_matrix"][ok]) - tv.unit_f(b["essential_matrix"][ok])).max()]
    for k in ("rotation", "position"):
        d.append(np.abs(a[k][ok] - b[k][ok]).max())
    return float(max(d))
