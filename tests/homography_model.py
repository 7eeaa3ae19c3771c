"""numpy restatement of tmi_ba_estimate_homographies, steps 2 to 7 (include/theia_mi355_ba.h): the stateless sampler,
the normalised four-point homography, the asymmetric transfer error, the integer cost or the MLESAC cost in its fixed
summation shape, the replay of SampleConsensusEstimator::Estimate's loop and the final inlier mask.

Every expression of steps 3 to 5 is written in the order the device kernels evaluate it (homography_kernels.h,
ransac_core.h), in IEEE double arithmetic without contraction (Python floats for the scalars, numpy arrays for the
per-correspondence residuals), with + - * / and sqrt only, so that the model's numbers are the device's bit for bit.
ComputeMaxIterations and the confidence use math.log / math.pow, the C library functions the engine's host side calls.

Two paths:
  "closed"  what the device does: the null vector by elimination with full pivoting, the MLE cost as 64 lane sums
            combined by the xor butterfly with offsets 32, 16, 8, 4, 2, 1
  "numpy"   the null vector of the 8x9 matrix through numpy.linalg.svd (the rank test stays the elimination's), the MLE
            cost through np.sum

Per hypothesis the DECISION MARGINS are recorded (Hypothesis.margins), each relative, so that "below 1e-9" means "a
rounding error could turn the decision":
  rank      |ratio - t| / t for ratio = |smallest pivot| / |largest pivot| and t = 8 DBL_EPSILON
  residual  min over the correspondences of |r - threshold| / threshold
  replay    of the comparison cost < best at the hypothesis' turn: |cost - best| / max(|cost|, |best|) under MLE.  Two
            costs that are bitwise equal are a decided "not less" (margin inf), as is any comparison of two integers and
            the comparison with the initial best."""
from __future__ import annotations

import math

import numpy as np

from localization_model import MASK64, _div, _sqrt, splitmix64_word

F = float
EPS = 2.220446049250313e-16
RANK_THRESHOLD = 8.0 * EPS
SQRT2 = 1.4142135623730951
DBL_MAX = 1.7976931348623157e308
MARGIN = 1e-9


# ---- the sampler -------------------------------------------------------------------------------------------------------
def sample(seed: int, p: int, i: int, n: int):
    """The sample of iteration i of stream p among n correspondences: four swaps of a partial Fisher-Yates."""
    a = {}
    for k in range(4):
        c = (4 * ((p << 32) + i) + k) & MASK64
        u = (float(splitmix64_word(seed, c) >> 11) + 0.5) * (1.0 / 9007199254740992.0)
        j = min(k + int(u * float(n - k)), n - 1)
        ak, aj = a.get(k, k), a.get(j, j)
        a[k], a[j] = aj, ak
    return tuple(a[k] for k in range(4))


def compute_max_iterations(inlier_ratio: float, log_failure_prob: float, min_iterations: int, max_iterations: int) -> int:
    """sample_consensus_estimator.h:215-243 for a sample of four without the T(d,d) test."""
    if inlier_ratio == 1.0:
        return min_iterations
    log_prob = math.log(1.0 - math.pow(inlier_ratio, 4.0)) - np.finfo(np.float64).eps
    num_iterations = log_failure_prob / log_prob
    return int(max(float(min_iterations), min(num_iterations, float(max_iterations))))


# ---- the hypothesis ----------------------------------------------------------------------------------------------------
def normalization(x, y):
    """(nf, cx, cy) of four points."""
    sx, sy = x[0], y[0]
    for k in range(1, 4):
        sx = sx + x[k]
        sy = sy + y[k]
    cx, cy = sx / 4.0, sy / 4.0
    ss = 0.0
    for k in range(4):
        dx, dy = x[k] - cx, y[k] - cy
        ss = ss + (dx * dx + dy * dy)
    rms = _sqrt(ss / 4.0)
    return _div(SQRT2, rms), cx, cy


def action_rows(x1, y1, x2, y2, n1, n2):
    """The 8x9 rows of CreateActionConstraint on the normalised points."""
    nf1, cx1, cy1 = n1
    nf2, cx2, cy2 = n2
    tx1, ty1, tx2, ty2 = -(nf1 * cx1), -(nf1 * cy1), -(nf2 * cx2), -(nf2 * cy2)
    A = []
    for k in range(4):
        a, b = nf1 * x1[k] + tx1, nf1 * y1[k] + ty1
        c, d = nf2 * x2[k] + tx2, nf2 * y2[k] + ty2
        A.append([0.0, 0.0, 0.0, -a, -b, -1.0, a * d, b * d, d])
        A.append([a, b, 1.0, 0.0, 0.0, 0.0, -(a * c), -(b * c), -c])
    return A


def eliminate(A):
    """The null vector of the 8x9 matrix A by elimination with full pivoting.  Returns (h [9] or None, pivot ratio)."""
    A = [list(r) for r in A]
    perm = list(range(9))
    max_pivot = min_pivot = 0.0
    for k in range(8):
        big, pr, pc = -1.0, k, k
        for r in range(k, 8):
            for c in range(k, 9):
                m = abs(A[r][c])
                if m > big:
                    big, pr, pc = m, r, c
        if not big > 0.0:
            return None, 0.0
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
        return None, ratio
    z = [0.0] * 9
    z[8] = 1.0
    for k in range(7, -1, -1):
        acc = 0.0
        for c in range(k + 1, 9):
            acc = acc + A[k][c] * z[c]
        z[k] = _div(-acc, A[k][k])
    h = [0.0] * 9
    for c in range(9):
        h[perm[c]] = z[c]
    return h, ratio


def unit_null_vector(h):
    ss, big, lead = 0.0, -1.0, 0.0
    for c in range(9):
        ss = ss + h[c] * h[c]
        m = abs(h[c])
        if m > big:
            big, lead = m, h[c]
    nrm = _sqrt(ss)
    if lead < 0.0:
        nrm = -nrm
    return [_div(h[c], nrm) for c in range(9)]


class Hypothesis:
    """One sample's model: H [9] row-major -- or none, with the reason."""

    def __init__(self):
        self.ok = False
        self.reason = ""
        self.margins = dict(rank=math.inf, residual=math.inf, replay=math.inf)
        self.cost = -1            # the integer cost: outliers (n - inliers under MLE)
        self.cost_real = math.nan  # the MLE cost

    def min_margin(self):
        return min(self.margins.values())


def hypothesis(x1, y1, x2, y2, path="closed"):
    """Step 3 for four correspondences (sequences of Python floats)."""
    h = Hypothesis()
    n1, n2 = normalization(x1, y1), normalization(x2, y2)
    if not n1[0] <= DBL_MAX or not n2[0] <= DBL_MAX:
        h.reason = "normalization"
        return h
    A = action_rows(x1, y1, x2, y2, n1, n2)
    v, ratio = eliminate(A)
    h.margins["rank"] = abs(ratio - RANK_THRESHOLD) / RANK_THRESHOLD if math.isfinite(ratio) else math.inf
    if v is None:
        h.reason = "rank"
        return h
    if path != "closed":
        v = [F(t) for t in np.linalg.svd(np.array(A))[2][8]]
    v = unit_null_vector(v)
    (nf1, cx1, cy1), (nf2, cx2, cy2) = n1, n2
    tx1, ty1 = -(nf1 * cx1), -(nf1 * cy1)
    inv2 = _div(1.0, nf2)
    G = [[v[3 * r] * nf1, v[3 * r + 1] * nf1, (v[3 * r] * tx1 + v[3 * r + 1] * ty1) + v[3 * r + 2]] for r in range(3)]
    h.H = [inv2 * G[0][c] + cx2 * G[2][c] for c in range(3)] + [inv2 * G[1][c] + cy2 * G[2][c] for c in range(3)] + \
        [G[2][c] for c in range(3)]
    h.ok = True
    return h


def residuals(H, X1, Y1, X2, Y2):
    """Step 4 over numpy arrays."""
    with np.errstate(all="ignore"):
        p0 = (H[0] * X1 + H[1] * Y1) + H[2]
        p1 = (H[3] * X1 + H[4] * Y1) + H[5]
        p2 = (H[6] * X1 + H[7] * Y1) + H[8]
        dx, dy = X2 - p0 / p2, Y2 - p1 / p2
        return dx * dx + dy * dy


def wave_sum(v):
    """The fixed summation shape of step 5: lane l of 64 adds v[l], v[l + 64], .. in ascending order from +0.0, then the
    xor butterfly with offsets 32, 16, 8, 4, 2, 1."""
    v = np.asarray(v, dtype=np.float64)
    rows = -(-v.size // 64)
    padded = np.zeros(max(rows, 1) * 64)  # (x + 0.0 == x for the x >= 0 summed here: the padding adds nothing)
    padded[:v.size] = v
    acc = np.zeros(64)
    for row in padded.reshape(-1, 64):
        acc = acc + row
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[lanes ^ off]
    assert (acc == acc[0]).all() or np.isnan(acc).all()
    return F(acc[0])


def score(h, X1, Y1, X2, Y2, thresh, path="closed"):
    """Steps 4 and 5: (inlier mask, MLE cost, smallest residual margin)."""
    r = residuals(h.H, X1, Y1, X2, Y2)
    with np.errstate(all="ignore"):
        inlier = r < thresh
        terms = np.where(inlier, r, thresh)
        mle = wave_sum(terms) if path == "closed" else F(np.sum(terms))
        m = np.abs(r - thresh) / thresh
        m = float(np.nanmin(m)) if np.isfinite(m).any() else math.inf
    return inlier, mle, m


# ---- RANSAC ------------------------------------------------------------------------------------------------------------
class RansacResult:
    pass


def ransac(f1, f2, thresh, p=0, seed=0, samples=None, failure_probability=0.01, min_inlier_ratio=0.0, min_iterations=10,
           max_iterations=1000, use_mle=False, path="closed", chunk=None):
    """Steps 2 to 7 for one pair with n >= 4.  f1, f2 [n, 2]; samples [max_iterations, 4] or None.  chunk: None runs the
    sequential loop as the reference writes it; an integer evaluates the iterations chunk by chunk against the bound at
    the chunk's start and replays them, as the device does."""
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
    res.hyp = {}            # iteration -> Hypothesis (with .cost, .cost_real)
    res.bound_changers = set()
    best_cost, best, best_it = None, None, -1

    def evaluate(i):
        s = samples[i] if samples is not None else sample(seed, p, i, n)
        s = [int(k) for k in s]
        h = hypothesis([F(X1[k]) for k in s], [F(Y1[k]) for k in s], [F(X2[k]) for k in s], [F(Y2[k]) for k in s], path)
        if h.ok:
            inlier, mle, m = score(h, X1, Y1, X2, Y2, thresh, path)
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
            if h.inliers < 4:  # inlier_ratio < 4 / n
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
        res.inlier_mask = score(best, X1, Y1, X2, Y2, thresh, path)[0]
    res.num_inliers = int(np.count_nonzero(res.inlier_mask))
    res.confidence = 1.0 - math.pow(1.0 - math.pow(res.num_inliers / n, 4.0), float(it))
    res.flagged = {i for i, h in res.hyp.items() if h.min_margin() < MARGIN}
    return res


def estimate(pair_offset, feature1, feature2, thresholds, pair_mask=None, pair_stream=None, samples=None, seed=0,
             path="closed", chunk=None, **kw):
    """Steps 1 to 7 for every selected pair.  Returns a dict of per-pair arrays like lib.estimate_homographies plus
    `results` {pair: RansacResult} and `flagged` [num_selected, max_iterations] bool."""
    po = np.asarray(pair_offset, dtype=np.int64)
    P = po.shape[0] - 1
    K = kw.get("max_iterations", 1000)
    f1 = np.asarray(feature1, dtype=np.float64).reshape(-1, 2)
    f2 = np.asarray(feature2, dtype=np.float64).reshape(-1, 2)
    sel = [p for p in range(P) if pair_mask is None or pair_mask[p]]
    out = dict(status=np.full(P, -1, np.int8), num_correspondences=np.zeros(P, np.int32),
               num_inliers=np.zeros(P, np.int32), num_iterations=np.zeros(P, np.int32),
               best_iteration=np.full(P, -1, np.int32), confidence=np.zeros(P), homography=np.zeros((P, 9)),
               corr_inlier=np.zeros(int(po[-1]), np.uint8), hypothesis_cost=np.full((len(sel), K), -1, np.int32),
               hypothesis_cost_real=np.full((len(sel), K), np.nan), flagged=np.zeros((len(sel), K), bool), results={})
    for rank, p in enumerate(sel):
        a, b = int(po[p]), int(po[p + 1])
        n = b - a
        out["num_correspondences"][p] = n
        if n < 4:
            out["status"][p] = 1
            continue
        r = ransac(f1[a:b], f2[a:b], float(thresholds[p]), p=p if pair_stream is None else int(pair_stream[p]),
                   seed=seed, samples=None if samples is None else samples[p], path=path, chunk=chunk, **kw)
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
        out["homography"][p] = np.array(r.best.H).reshape(3, 3).T.reshape(9)  # column-major
    return out


def unit_h(h_column_major):
    """H [.., 9] column-major -> [.., 3, 3] with unit Frobenius norm and its largest-magnitude entry positive."""
    Hm = np.asarray(h_column_major, dtype=np.float64).reshape(-1, 3, 3).transpose(0, 2, 1).copy()
    for k in range(Hm.shape[0]):
        nrm = np.linalg.norm(Hm[k])
        if nrm > 0:
            Hm[k] /= nrm
            i = np.argmax(np.abs(Hm[k]))
            if Hm[k].flat[i] < 0:
                Hm[k] = -Hm[k]
    return Hm


def model_spread(a, b):
    """MODEL_SPREAD of two outputs of estimate() (or of the device): the largest difference in H (unit Frobenius norm,
    sign fixed) and the confidence over the pairs both estimated."""
    ok = (a["status"] == 0) & (b["status"] == 0)
    if not ok.any():
        return 0.0
    return float(max(np.abs(unit_h(a["homography"][ok]) - unit_h(b["homography"][ok])).max(),
                     np.abs(a["confidence"][ok] - b["confidence"][ok]).max()))
