"""numpy restatement of theia::NonlinearRotationEstimator (nonlinear_rotation_estimator.cc:49-100,
pairwise_rotation_error.h:65-95) under Ceres 1.14's SoftLOneLoss, Corrector, TrustRegionMinimizer and
LevenbergMarquardtStrategy, in the fixed orders of tmi_ba_estimate_global_rotations_nonlinear
(include/theia_mi355_ba.h).  Written from the reference's functor, Ceres' rotation.h and Ceres' rules:

  * the residual and its 3 x 6 Jacobian come from forward-mode dual numbers (class Dual, arrays over the edges) through
    AngleAxisToRotationMatrix, the two matrix products in the reference's order (R2 R1^T) Rrel^T, RotationMatrixToQuaternion
    and QuaternionToAngleAxis, every branch selected per edge on the values as Ceres' Jets select it;
  * SoftLOneLoss and the corrector's shortcut (rho'' < 0 everywhere, asserted);
  * the problem: edges between marked views in the caller's order, the marked views with such an edge in ascending index,
    a held view's rows and columns removed;
  * the normal equations J~^T J~ y = J~^T r~ block by block, every per-view sum from zero in ascending edge index, Jacobi
    scaling from the first linearisation, the LM diagonal clamp(A_ii, lo, hi) / radius;
  * two linear-solve paths: `own`, a column-by-column Cholesky written here (pivot j = A_jj minus the squares of row j of
    the factor so far), and `linalg`, numpy.linalg.cholesky;
  * every scalar by the reduction of fixed shape of the other models (fixed_sum).

Every decision of the loop is recorded with its margin, the relative distance of the compared value from its threshold;
a pivot's margin is the pivot over the diagonal entry it came from.
"""
import numpy as np
import scipy.linalg

from robust_rotation_model import _margin, _sq3, fixed_sum

# nonlinear_rotation_estimator.h / .cc:94 and ceres::Solver::Options
DEFAULTS = dict(max_num_iterations=200, robust_loss_width=0.1, fixed_view=-1, jacobi_scaling=1,
                max_num_consecutive_invalid_steps=5, function_tolerance=1e-6, gradient_tolerance=1e-10,
                parameter_tolerance=1e-8, initial_trust_region_radius=1e4, max_trust_region_radius=1e16,
                min_trust_region_radius=1e-32, min_relative_decrease=1e-3, min_lm_diagonal=1e-6, max_lm_diagonal=1e32)
DBL_MIN = 2.2250738585072014e-308
DBL_EPSILON = 2.220446049250313e-16


# ---- dual numbers over arrays: a [E], v [E, N] ---------------------------------------------------------------------------
class Dual:
    def __init__(self, a, v):
        self.a, self.v = a, v

    @staticmethod
    def const(c, like):
        return Dual(np.broadcast_to(np.asarray(c, dtype=np.float64), like.a.shape).copy(), np.zeros_like(like.v))

    def _lift(self, o):
        return o if isinstance(o, Dual) else Dual.const(o, self)

    def __add__(self, o):
        o = self._lift(o)
        return Dual(self.a + o.a, self.v + o.v)

    def __sub__(self, o):
        o = self._lift(o)
        return Dual(self.a - o.a, self.v - o.v)

    def __neg__(self):
        return Dual(-self.a, -self.v)

    def __mul__(self, o):
        o = self._lift(o)
        return Dual(self.a * o.a, self.a[:, None] * o.v + self.v * o.a[:, None])

    __radd__, __rmul__ = __add__, __mul__

    def __truediv__(self, o):  # Ceres' Jet division
        o = self._lift(o)
        gi = 1.0 / o.a
        fr = self.a * gi
        return Dual(fr, (self.v - fr[:, None] * o.v) * gi[:, None])


def dsqrt(f):
    t = np.sqrt(f.a)
    return Dual(t, f.v * (1.0 / (2.0 * t))[:, None])


def dsin(f):
    return Dual(np.sin(f.a), np.cos(f.a)[:, None] * f.v)


def dcos(f):
    return Dual(np.cos(f.a), -np.sin(f.a)[:, None] * f.v)


def datan2(g, f):
    tmp = 1.0 / (f.a * f.a + g.a * g.a)
    return Dual(np.arctan2(g.a, f.a), tmp[:, None] * (f.a[:, None] * g.v - g.a[:, None] * f.v))


def where(mask, x, y):
    return Dual(np.where(mask, x.a, y.a), np.where(mask[:, None], x.v, y.v))


def variables(x, first, count):
    """x [E, 3] as three Duals whose derivative k is slot first + k of `count`."""
    out = []
    for k in range(3):
        v = np.zeros((x.shape[0], count))
        v[:, first + k] = 1.0
        out.append(Dual(x[:, k].astype(np.float64), v))
    return out


# ---- Ceres' rotation.h on Duals; matrices are R[r][c] --------------------------------------------------------------------
def angle_axis_to_matrix(aa):
    """ceres::AngleAxisToRotationMatrix; returns (R, the mask of the theta^2 > epsilon branch)."""
    one = Dual.const(1.0, aa[0])
    theta2 = aa[0] * aa[0] + aa[1] * aa[1] + aa[2] * aa[2]
    big = theta2.a > DBL_EPSILON
    with np.errstate(all="ignore"):
        theta = dsqrt(theta2)
        wx, wy, wz = aa[0] / theta, aa[1] / theta, aa[2] / theta
        c, s = dcos(theta), dsin(theta)
        omc = one - c
        far = [[c + wx * wx * omc, wx * wy * omc - wz * s, wy * s + wx * wz * omc],
               [wz * s + wx * wy * omc, c + wy * wy * omc, -(wx * s) + wy * wz * omc],
               [-(wy * s) + wx * wz * omc, wx * s + wy * wz * omc, c + wz * wz * omc]]
    near = [[one, -aa[2], aa[1]], [aa[2], one, -aa[0]], [-aa[1], aa[0], one]]
    return [[where(big, far[r][c_], near[r][c_]) for c_ in range(3)] for r in range(3)], big


def matmul_t(A, B):
    """A B^T"""
    return [[A[r][0] * B[c][0] + A[r][1] * B[c][1] + A[r][2] * B[c][2] for c in range(3)] for r in range(3)]


def matrix_to_angle_axis(R):
    """ceres::RotationMatrixToAngleAxis = RotationMatrixToQuaternion + QuaternionToAngleAxis; returns (aa, branch) with
    branch [E] in 0 (trace >= 0), 1, 2, 3 (largest diagonal entry 0, 1, 2), plus 4 where sin^2 = 0 (k = 2) and 8 where
    the scalar part is negative."""
    trace = R[0][0] + R[1][1] + R[2][2]
    with np.errstate(all="ignore"):
        t = dsqrt(trace + 1.0)
        q_trace = [t * 0.5]
        t = Dual.const(0.5, t) / t
        q_trace += [(R[2][1] - R[1][2]) * t, (R[0][2] - R[2][0]) * t, (R[1][0] - R[0][1]) * t]
        q_diag = []
        for i in range(3):
            j = (i + 1) % 3
            k = (j + 1) % 3
            t = dsqrt(R[i][i] - R[j][j] - R[k][k] + 1.0)
            q = [None] * 4
            q[i + 1] = t * 0.5
            t = Dual.const(0.5, t) / t
            q[0] = (R[k][j] - R[j][k]) * t
            q[j + 1] = (R[j][i] + R[i][j]) * t
            q[k + 1] = (R[k][i] + R[i][k]) * t
            q_diag.append(q)
    i = np.zeros(trace.a.shape, dtype=np.int64)
    i[R[1][1].a > R[0][0].a] = 1
    largest = np.where(i == 1, R[1][1].a, R[0][0].a)
    i[R[2][2].a > largest] = 2
    branch = np.where(trace.a >= 0.0, 0, i + 1)
    q = [where(branch == 0, q_trace[m], where(branch == 1, q_diag[0][m], where(branch == 2, q_diag[1][m], q_diag[2][m])))
         for m in range(4)]
    s2 = q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
    positive = s2.a > 0.0
    negative = q[0].a < 0.0
    with np.errstate(all="ignore"):
        s = dsqrt(s2)
        two_theta = where(negative, datan2(-s, -q[0]), datan2(s, q[0])) * 2.0
        k = where(positive, two_theta / s, Dual.const(2.0, s))
    return [q[1] * k, q[2] * k, q[3] * k], branch + 4 * (~positive) + 8 * (negative & positive)


def pairwise_rotation_error(x1, x2, rel):
    """The reference's functor on arrays [E, 3]: r [E, 3], J [E, 3, 6] (x1's columns first), and the branches taken:
    (first-order branch of R1, of R2, the code of matrix_to_angle_axis)."""
    E = x1.shape[0]
    a1, a2 = variables(x1, 0, 6), variables(x2, 3, 6)
    R1, big1 = angle_axis_to_matrix(a1)
    R2, big2 = angle_axis_to_matrix(a2)
    zero = Dual(np.zeros(E), np.zeros((E, 6)))
    Rrel, _ = angle_axis_to_matrix([zero + rel[:, k] for k in range(3)])
    err, code = matrix_to_angle_axis(matmul_t(matmul_t(R2, R1), Rrel))
    r = np.stack([e.a for e in err], axis=1)
    J = np.stack([e.v for e in err], axis=1)
    return r, J, (~big1, ~big2, code)


def soft_l_one(s, a):
    """ceres::SoftLOneLoss::Evaluate: rho, rho', rho'' per item."""
    b = a * a
    c = 1.0 / b
    total = 1.0 + s * c
    tmp = np.sqrt(total)
    rho1 = np.maximum(DBL_MIN, 1.0 / tmp)
    return 2.0 * b * (tmp - 1.0), rho1, -(c * rho1) / (2.0 * total)


def corrected(r, J, width):
    """Ceres' Corrector: (rho, r~, J~).  rho'' < 0 everywhere, so the shortcut sqrt(rho') on both is all there is."""
    rho0, rho1, rho2 = soft_l_one(_sq3(r), width)
    assert (rho2 < 0.0).all()
    sq = np.sqrt(rho1)
    return rho0, sq[:, None] * r, sq[:, None, None] * J


# ---- the problem ---------------------------------------------------------------------------------------------------------
class Problem:
    def __init__(self, num_views, view1, view2, rel, view_given, fixed_view):
        view1, view2 = np.asarray(view1, dtype=np.int64), np.asarray(view2, dtype=np.int64)
        given = np.ones(num_views, dtype=bool) if view_given is None else np.asarray(view_given).astype(bool)
        self.used = np.flatnonzero(given[view1] & given[view2])  # the caller's indices of the edges used
        self.views = np.unique(np.concatenate([view1[self.used], view2[self.used]]))
        index = -np.ones(num_views, dtype=np.int64)
        index[self.views] = np.arange(self.views.size)
        self.v1, self.v2 = index[view1[self.used]], index[view2[self.used]]
        self.rel = np.asarray(rel, dtype=np.float64)[self.used]
        self.Vp, self.E = self.views.size, self.used.size
        self.held = int(index[fixed_view]) if fixed_view >= 0 and index[fixed_view] >= 0 else -1
        self.free = np.array([p for p in range(self.Vp) if p != self.held], dtype=np.int64)
        self.n = self.free.size
        self.ends = np.stack([self.v1, self.v2], axis=1).ravel()  # per view in ascending edge index


def linearize(P, full, width):
    """At the rotations `full` [Vp, 3]: cost, r, the record (B11, B22, B12, q1, q2) and the branches."""
    r, J, branches = pairwise_rotation_error(full[P.v1], full[P.v2], P.rel)
    rho0, rt, Jt = corrected(r, J, width)
    J1, J2 = Jt[:, :, :3], Jt[:, :, 3:]
    rec = (np.einsum("eki,ekj->eij", J1, J1), np.einsum("eki,ekj->eij", J2, J2), np.einsum("eki,ekj->eij", J1, J2),
           np.einsum("eki,ek->ei", J1, rt), np.einsum("eki,ek->ei", J2, rt))
    return fixed_sum(0.5 * rho0), r, rec, branches


def cost_at(P, full, width):
    r = pairwise_rotation_error(full[P.v1], full[P.v2], P.rel)[0]
    return fixed_sum(0.5 * soft_l_one(_sq3(r), width)[0])


def view_diagonal(P, rec):
    """per problem view the 3 x 3 diagonal block, summed from zero in ascending edge index"""
    diag = np.zeros((P.Vp, 3, 3))
    np.add.at(diag, P.ends, np.stack([rec[0], rec[1]], axis=1).reshape(-1, 3, 3))
    return diag


def normal_equations(P, rec, scale):
    """The scaled normal matrix [3 n, 3 n], the scaled gradient and the unscaled one ([n, 3]); scale [n, 3]."""
    blocks = np.zeros((P.Vp, P.Vp, 3, 3))
    blocks[P.v1, P.v2] = rec[2]  # (no unordered pair appears twice)
    blocks[P.v2, P.v1] = rec[2].transpose(0, 2, 1)
    blocks[np.arange(P.Vp), np.arange(P.Vp)] = view_diagonal(P, rec)
    blocks = blocks[P.free][:, P.free]
    A = blocks.transpose(0, 2, 1, 3).reshape(3 * P.n, 3 * P.n)
    s = scale.ravel()
    A = (A * s[:, None]) * s[None, :]
    grad = np.zeros((P.Vp, 3))
    np.add.at(grad, P.ends, np.stack([rec[3], rec[4]], axis=1).reshape(-1, 3))
    grad = grad[P.free]
    return A, grad * scale, grad


def cholesky_own(A):
    """Column by column; returns (L, the smallest pivot / diagonal entry).  LinAlgError on a non-positive pivot."""
    n = A.shape[0]
    L = np.zeros_like(A)
    smallest = np.inf
    for j in range(n):
        c = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not c[0] > 0.0:
            raise np.linalg.LinAlgError("pivot %d" % j)
        smallest = min(smallest, c[0] / A[j, j])
        L[j, j] = np.sqrt(c[0])
        L[j + 1:, j] = c[1:] / L[j, j]
    return L, smallest


def solve(A, rhs, path):
    if path == "own":
        L, smallest = cholesky_own(A)
    else:
        L = np.linalg.cholesky(A)
        d = np.diag(L)
        smallest = float((d * d / np.diag(A)).min())
    y = scipy.linalg.solve_triangular(L, rhs, lower=True)
    return scipy.linalg.solve_triangular(L.T, y, lower=False), smallest


def estimate(num_views, view1, view2, relative_rotations, view_rotation, view_given=None, options=None, path="own"):
    """Returns a dict: rotations [V, 3] (views outside the problem and the held view as given), residuals [E, 3] (0 for a
    skipped edge), costs, radii, outcomes (entry 0 the start, then one per iteration run: 1 accepted, 0 rejected, -1
    invalid, 2 / 3 ended by the parameter / function tolerance), iterations, termination (0 CONVERGENCE, 1 NO_CONVERGENCE,
    2 FAILURE), factorizations, margins, min_margin, num_views, num_pairs, and `branches`, the set of
    (first-order R1, first-order R2, code of matrix_to_angle_axis) triples seen at any linearisation."""
    opt = dict(DEFAULTS)
    opt.update(options or {})
    start = np.array(view_rotation, dtype=np.float64).reshape(-1, 3)
    P = Problem(num_views, view1, view2, relative_rotations, view_given, int(opt["fixed_view"]))
    n, width = P.n, opt["robust_loss_width"]
    full = start[P.views].copy()
    x = full[P.free]
    seen = set()

    def place(x):
        out = full.copy()
        out[P.free] = x
        return out

    def lin(x):
        cost, r, rec, (f1, f2, code) = linearize(P, place(x), width)
        seen.update(zip(f1.tolist(), f2.tolist(), code.tolist()))
        return cost, r, rec

    cost, r, rec = lin(x)
    scale = np.ones((n, 3))
    if opt["jacobi_scaling"]:
        d = view_diagonal(P, rec)[:, [0, 1, 2], [0, 1, 2]]
        scale = 1.0 / (1.0 + np.sqrt(d[P.free]))
    A, grad, grad_unscaled = normal_equations(P, rec, scale)
    x_norm = np.sqrt(fixed_sum(x.ravel() * x.ravel()))
    radius, decrease_factor = opt["initial_trust_region_radius"], 2.0
    invalid_run, it, termination, factorizations = 0, 0, 1, 0
    need_gradient_check = True
    costs, radii, outcomes, margins = [cost], [radius], [1], []

    def record(outcome):
        costs.append(cost)
        radii.append(radius)
        outcomes.append(outcome)

    while it < opt["max_num_iterations"]:
        it += 1
        gn = np.diag(A).copy()
        damped = A.copy()
        damped[np.arange(3 * n), np.arange(3 * n)] = gn + np.minimum(np.maximum(gn, opt["min_lm_diagonal"]),
                                                                     opt["max_lm_diagonal"]) / radius
        factorizations += 1
        usable = True
        try:
            y, pivot_margin = solve(damped, grad.ravel(), path)
            y = y.reshape(n, 3)
            margins.append(pivot_margin)
        except np.linalg.LinAlgError:
            usable, y = False, np.zeros((n, 3))
            margins.append(0.0)
        if need_gradient_check:
            need_gradient_check = False
            gmax = float(np.abs(grad_unscaled).max())
            margins.append(_margin(gmax, opt["gradient_tolerance"]))
            if not gmax > opt["gradient_tolerance"]:
                termination = 0
                it -= 1
                break
        step = -(scale * y)
        cand = x + step
        sfull = np.zeros((P.Vp, 3))
        sfull[P.free] = step
        s1, s2 = sfull[P.v1], sfull[P.v2]
        quad = (np.einsum("ei,eij,ej->e", s1, rec[0], s1) + 2.0 * np.einsum("ei,eij,ej->e", s1, rec[2], s2)) + \
            np.einsum("ei,eij,ej->e", s2, rec[1], s2)
        mcc_edges = -((np.einsum("ei,ei->e", s1, rec[3]) + np.einsum("ei,ei->e", s2, rec[4])) + 0.5 * quad)
        mcc = fixed_sum(mcc_edges)
        cand_cost = cost_at(P, place(cand), width)
        step_sq = fixed_sum(step.ravel() * step.ravel())
        cand_x_sq = fixed_sum(cand.ravel() * cand.ravel())
        if usable:
            # model_cost_change > 0: the threshold is 0, so the sum is held against the size of its terms
            margins.append(abs(mcc) / max(float(np.abs(mcc_edges).sum()), DBL_MIN))
        if not mcc > 0.0:
            usable = False
        if not usable:
            invalid_run += 1
            if invalid_run >= opt["max_num_consecutive_invalid_steps"]:
                record(-1)
                termination = 2
                break
            radius /= decrease_factor
            decrease_factor *= 2.0
            record(-1)
            margins.append(_margin(radius, opt["min_trust_region_radius"]))
            if radius < opt["min_trust_region_radius"]:
                termination = 0
                break
            continue
        invalid_run = 0
        step_norm, bound = np.sqrt(step_sq), opt["parameter_tolerance"] * (x_norm + opt["parameter_tolerance"])
        margins.append(_margin(step_norm, bound))
        if step_norm <= bound:
            record(2)
            termination = 0
            break
        cost_change = cost - cand_cost
        margins.append(_margin(abs(cost_change), opt["function_tolerance"] * cost))
        if abs(cost_change) <= opt["function_tolerance"] * cost:
            record(3)
            termination = 0
            break
        relative_decrease = cost_change / mcc
        margins.append(_margin(relative_decrease, opt["min_relative_decrease"]))
        if relative_decrease > opt["min_relative_decrease"]:
            x, cost, x_norm = cand, cand_cost, np.sqrt(cand_x_sq)
            radius = radius / max(1.0 / 3.0, 1.0 - (2.0 * relative_decrease - 1.0) ** 3)
            radius = min(opt["max_trust_region_radius"], radius)
            decrease_factor = 2.0
            _, r, rec = lin(x)
            A, grad, grad_unscaled = normal_equations(P, rec, scale)
            need_gradient_check = True
            record(1)
        else:
            radius /= decrease_factor
            decrease_factor *= 2.0
            record(0)
        margins.append(_margin(radius, opt["min_trust_region_radius"]))
        if radius < opt["min_trust_region_radius"]:
            termination = 0
            break
    rotations = start.copy()
    rotations[P.views] = place(x)
    residuals = np.zeros((np.asarray(view1).size, 3))
    residuals[P.used] = r
    return dict(rotations=rotations, residuals=residuals, costs=np.array(costs), radii=np.array(radii),
                outcomes=np.array(outcomes, dtype=np.int32), iterations=it, termination=termination,
                factorizations=factorizations, margins=margins, min_margin=min(margins) if margins else np.inf,
                num_views=P.Vp, num_pairs=P.E, branches=seen)


# ---- gauge-invariant comparison -------------------------------------------------------------------------------------------
def rotation_matrices(aa):
    """[V, 3] angle-axis to [V, 3, 3] (Rodrigues; for comparisons, not part of the model's arithmetic)."""
    aa = np.asarray(aa, dtype=np.float64)
    theta = np.linalg.norm(aa, axis=1)
    k = aa / np.where(theta > 0, theta, 1.0)[:, None]
    K = np.zeros((aa.shape[0], 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -k[:, 2], k[:, 1], k[:, 2], -k[:, 0], -k[:, 1], k[:, 0]
    return np.eye(3)[None] + np.sin(theta)[:, None, None] * K + (1.0 - np.cos(theta))[:, None, None] * (K @ K)


def loop_rotations(aa, view1, view2):
    """R2 R1^T per edge [E, 3, 3]: unchanged by R_v -> R_v Q."""
    R = rotation_matrices(aa)
    return R[view2] @ R[view1].transpose(0, 2, 1)


def aligned_rotation_difference(a, b, views):
    """The largest entry of |R_a(v) Q - R_b(v)| over `views`, Q the rotation that best maps a onto b (Procrustes)."""
    Ra, Rb = rotation_matrices(a)[views], rotation_matrices(b)[views]
    U, _, Vt = np.linalg.svd(np.einsum("vji,vjk->ik", Ra, Rb))
    Q = U @ np.diag([1.0, 1.0, np.linalg.det(U @ Vt)]) @ Vt
    return float(np.abs(Ra @ Q - Rb).max())


def gauge_invariant_difference(a, b, view1, view2, used_views, aligned=True):
    """The largest difference between two results (dicts of `estimate` or of the device call) over every real-valued
    gauge-invariant output: loop rotations of the edges used, residuals, costs and radii (relative to the larger entry),
    and, per connected graph, the rotations after alignment.  Traces of unequal length are compared on their common part."""
    used = np.flatnonzero(np.isin(view1, used_views) & np.isin(view2, used_views))
    out = float(np.abs(loop_rotations(a["rotations"], view1[used], view2[used]) -
                       loop_rotations(b["rotations"], view1[used], view2[used])).max())
    out = max(out, float(np.abs(a["residuals"] - b["residuals"]).max()))
    for key in ("costs", "radii"):
        m = min(a[key].size, b[key].size)
        scale = np.maximum(np.maximum(np.abs(a[key][:m]), np.abs(b[key][:m])), DBL_MIN)
        out = max(out, float((np.abs(a[key][:m] - b[key][:m]) / scale).max()))
    if aligned:
        out = max(out, aligned_rotation_difference(a["rotations"], b["rotations"], used_views))
    return out


# ---- scenes --------------------------------------------------------------------------------------------------------------
def random_rotations(n, scale, rng):
    return scale * rng.uniform(-1.0, 1.0, size=(n, 3))


def matrices_to_angle_axis(R):
    """[E, 3, 3] to angle-axis through this file's restatement of Ceres' code."""
    E = R.shape[0]
    zero = Dual(np.zeros(E), np.zeros((E, 1)))
    aa, _ = matrix_to_angle_axis([[zero + R[:, r, c] for c in range(3)] for r in range(3)])
    return np.stack([x.a for x in aa], axis=1)


def scene_on_pairs(num_views, pairs, noise, seed, outlier_fraction=0.0, scale=1.0):
    """Ground-truth rotations, and per pair rotation_2 = R2 R1^T perturbed on the left by a rotation of up to `noise`
    radians; a fraction of the pairs gets a uniformly random large error instead.  Returns (gt, view1, view2, rel)."""
    rng = np.random.default_rng(seed)
    gt = random_rotations(num_views, scale, rng)
    v1 = np.array([p[0] for p in pairs], dtype=np.int32)
    v2 = np.array([p[1] for p in pairs], dtype=np.int32)
    loop = loop_rotations(gt, v1, v2)
    err = noise * rng.uniform(-1.0, 1.0, size=(v1.size, 3))
    outlier = rng.random(v1.size) < outlier_fraction
    err[outlier] = random_rotations(int(outlier.sum()), 2.5, rng)
    rel = matrices_to_angle_axis(rotation_matrices(err) @ loop)
    return gt, v1, v2, rel


def random_pairs(num_views, num_pairs, rng):
    """A spanning chain 0-1-...-(V-1) first, then distinct random pairs, in random directions."""
    pairs = [(i - 1, i) for i in range(1, num_views)]
    seen = set(pairs)
    while len(pairs) < num_pairs:
        a, b = (int(x) for x in rng.integers(0, num_views, size=2))
        if a != b and (min(a, b), max(a, b)) not in seen:
            seen.add((min(a, b), max(a, b)))
            pairs.append((a, b) if rng.random() < 0.5 else (b, a))
    return pairs
