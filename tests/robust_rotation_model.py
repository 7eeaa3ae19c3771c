"""numpy restatement of theia::RobustRotationEstimator (robust_rotation_estimator.cc:66-282, math/l1_solver.h:120-178,
math/rotation.cc:122-132) in the fixed orders of tmi_ba_estimate_global_rotations_robust (include/theia_mi355_ba.h):

  * views are a dense table, `fixed_view` is held; free view v has column v - (v > fixed_view); n = V - 1;
  * A^T W A = L_w (x) I3: ONE symmetric positive definite system of order n with three right-hand sides, L_w the weighted
    graph Laplacian without the fixed view's row and column;
  * every per-view sum over a view's edges runs from zero in ascending edge index (np.add.at is unbuffered and applies
    its updates in the order given);
  * every sum over the edges or over the views is fixed_sum(): blocks of 256 consecutive items are added by a binary tree
    (item t += item t + half, half = 128 ... 1), the block sums are dealt to 256 accumulators (accumulator t takes block
    sums t, t + 256, ... in ascending order) and those are added by the same tree.

Two switches exist only to measure the model against itself: lu=True solves with an LU factorisation instead of Cholesky,
perm renumbers the views (the edges keep their order) and maps the result back.  Every decision the loops take is
recorded with its margin: |value - threshold| / threshold.
"""
import numpy as np
import scipy.linalg

DBL_EPSILON = 2.220446049250313e-16
DEFAULTS = dict(max_num_l1_iterations=5, l1_step_convergence_threshold=1e-3, max_num_irls_iterations=100,
                irls_step_convergence_threshold=1e-3, irls_loss_parameter_sigma=5.0 * np.pi / 180.0)
# math/l1_solver.h:89-98 as RobustRotationEstimator uses it: constants, not options
ADMM_FIRST_BUDGET, RHO, ALPHA, ABS_TOL, REL_TOL = 5, 1.0, 1.0, 1e-4, 1e-2


# ---- rotations (vectorised over the leading axis) ---------------------------------------------------------------------
def angle_axis_to_matrix(aa):
    """ceres::AngleAxisToRotationMatrix; returns [N, 3, 3] with M[:, r, c] = R(r, c)."""
    aa = np.asarray(aa, dtype=np.float64).reshape(-1, 3)
    theta2 = aa[:, 0] * aa[:, 0] + aa[:, 1] * aa[:, 1] + aa[:, 2] * aa[:, 2]
    big = theta2 > DBL_EPSILON
    theta = np.sqrt(np.where(big, theta2, 1.0))
    wx, wy, wz = aa[:, 0] / theta, aa[:, 1] / theta, aa[:, 2] / theta
    c, s = np.cos(theta), np.sin(theta)
    omc = 1.0 - c
    R = np.empty((aa.shape[0], 3, 3))
    R[:, 0, 0] = c + wx * wx * omc
    R[:, 1, 0] = wz * s + wx * wy * omc
    R[:, 2, 0] = -wy * s + wx * wz * omc
    R[:, 0, 1] = wx * wy * omc - wz * s
    R[:, 1, 1] = c + wy * wy * omc
    R[:, 2, 1] = wx * s + wy * wz * omc
    R[:, 0, 2] = wy * s + wx * wz * omc
    R[:, 1, 2] = -wx * s + wy * wz * omc
    R[:, 2, 2] = c + wz * wz * omc
    small = ~big
    if small.any():
        a = aa[small]
        S = np.zeros((a.shape[0], 3, 3))
        S[:, 0, 0] = S[:, 1, 1] = S[:, 2, 2] = 1.0
        S[:, 1, 0], S[:, 2, 0] = a[:, 2], -a[:, 1]
        S[:, 0, 1], S[:, 2, 1] = -a[:, 2], a[:, 0]
        S[:, 0, 2], S[:, 1, 2] = a[:, 1], -a[:, 0]
        R[small] = S
    return R


def matrix_to_angle_axis(R):
    """ceres::RotationMatrixToAngleAxis of Ceres 1.x: RotationMatrixToQuaternion, then QuaternionToAngleAxis."""
    R = np.asarray(R, dtype=np.float64).reshape(-1, 3, 3)
    N = R.shape[0]
    q = np.empty((N, 4))
    trace = R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]
    pos = trace >= 0.0
    t = np.sqrt(np.where(pos, trace, 0.0) + 1.0)
    q[:, 0] = 0.5 * t
    t = 0.5 / t
    q[:, 1] = (R[:, 2, 1] - R[:, 1, 2]) * t
    q[:, 2] = (R[:, 0, 2] - R[:, 2, 0]) * t
    q[:, 3] = (R[:, 1, 0] - R[:, 0, 1]) * t
    for m in np.nonzero(~pos)[0]:
        M = R[m]
        i = 0
        if M[1, 1] > M[0, 0]:
            i = 1
        if M[2, 2] > M[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        tt = np.sqrt(M[i, i] - M[j, j] - M[k, k] + 1.0)
        q[m, i + 1] = 0.5 * tt
        tt = 0.5 / tt
        q[m, 0] = (M[k, j] - M[j, k]) * tt
        q[m, j + 1] = (M[j, i] + M[i, j]) * tt
        q[m, k + 1] = (M[k, i] + M[i, k]) * tt
    s2 = q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3]
    nz = s2 > 0.0
    s = np.sqrt(np.where(nz, s2, 1.0))
    c = q[:, 0]
    two_theta = 2.0 * np.where(c < 0.0, np.arctan2(-s, -c), np.arctan2(s, c))
    k = np.where(nz, two_theta / s, 2.0)
    return q[:, 1:] * k[:, None]


def matmul3(A, B):
    """C(r, c) = (A(r, 0) B(0, c) + A(r, 1) B(1, c)) + A(r, 2) B(2, c)."""
    return (A[:, :, 0, None] * B[:, None, 0, :] + A[:, :, 1, None] * B[:, None, 1, :]) + A[:, :, 2, None] * B[:, None, 2, :]


def multiply_rotations(a, b):
    """theia::MultiplyRotations (math/rotation.cc:122-132): the angle-axis of R(a) R(b)."""
    return matrix_to_angle_axis(matmul3(angle_axis_to_matrix(a), angle_axis_to_matrix(b)))


# ---- fixed-shape sums -------------------------------------------------------------------------------------------------
def _tree256(a):
    a = a.copy()
    half = 128
    while half > 0:
        a[:, :half] += a[:, half:2 * half]
        half >>= 1
    return a[:, 0]


def fixed_sum(x):
    x = np.asarray(x, dtype=np.float64).ravel()
    nb = max((x.size + 255) // 256, 1)
    pad = np.zeros(nb * 256)
    pad[:x.size] = x
    part = _tree256(pad.reshape(nb, 256))
    acc = np.zeros(256)
    for k in range(0, nb, 256):  # accumulator t: block sums t, t + 256, ... in ascending order
        chunk = part[k:k + 256]
        acc[:chunk.size] += chunk
    return float(_tree256(acc.reshape(1, 256))[0])


def _sq3(x):
    """per item x0^2 + x1^2 + x2^2, left to right"""
    return (x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2]


# ---- the graph --------------------------------------------------------------------------------------------------------
class Graph:
    def __init__(self, num_views, view1, view2, fixed_view):
        self.V = int(num_views)
        self.v1 = np.asarray(view1, dtype=np.int64)
        self.v2 = np.asarray(view2, dtype=np.int64)
        self.E = self.v1.size
        self.fixed = int(fixed_view)
        self.n = self.V - 1
        col = np.arange(self.V) - (np.arange(self.V) > self.fixed)
        col[self.fixed] = -1
        self.col = col
        self.c1, self.c2 = col[self.v1], col[self.v2]
        # (view, sign) of both ends of every edge, edge-major: per view the entries come in ascending edge index
        self.ends = np.stack([self.v1, self.v2], axis=1).ravel()
        self.signs = np.tile(np.array([-1.0, 1.0]), self.E)

    def At(self, y):
        """A^T y per free view ([n, 3]) for y [E, 3]: every view's sum from zero in ascending edge index."""
        out = np.zeros((self.V, 3))
        np.add.at(out, self.ends, np.repeat(y, 2, axis=0) * self.signs[:, None])
        return np.delete(out, self.fixed, axis=0)

    def A(self, x):
        """A x per edge for x [n, 3]."""
        full = np.insert(x, self.fixed, 0.0, axis=0)
        return full[self.v2] - full[self.v1]

    def laplacian(self, w=None):
        """The reduced weighted Laplacian [n, n]; parallel edges add in ascending edge index."""
        w = np.ones(self.E) if w is None else w
        diag = np.zeros(self.V)
        np.add.at(diag, self.ends, np.repeat(w, 2))
        L = np.zeros((self.n, self.n))
        both = (self.c1 >= 0) & (self.c2 >= 0)
        a, b, ww = self.c1[both], self.c2[both], w[both]
        off = np.zeros((self.n, self.n))
        np.add.at(off, (np.stack([a, b], axis=1).ravel(), np.stack([b, a], axis=1).ravel()), np.repeat(ww, 2))
        L -= off
        L[np.arange(self.n), np.arange(self.n)] = np.delete(diag, self.fixed)
        return L


class _Solver:
    def __init__(self, L, lu):
        self.lu = lu
        if lu:
            self.f = scipy.linalg.lu_factor(L)
        else:
            self.f = np.linalg.cholesky(L)  # raises LinAlgError on a non-positive pivot

    def solve(self, rhs):
        if self.lu:
            return scipy.linalg.lu_solve(self.f, rhs)
        y = scipy.linalg.solve_triangular(self.f, rhs, lower=True)
        return scipy.linalg.solve_triangular(self.f.T, y, lower=False)


def _margin(value, threshold):
    return abs(value - threshold) / threshold if threshold > 0 else np.inf


def compute_residuals(g, rel, o):
    """ComputeResiduals (:256-272)"""
    return multiply_rotations(-o[g.v2], multiply_rotations(rel, o[g.v1]))


def update_rotations(g, o, step):
    """UpdateGlobalRotations (:240-252) and ComputeAverageStepSize (:274-282)"""
    free = np.arange(g.V) != g.fixed
    o = o.copy()
    o[free] = multiply_rotations(o[free], step)
    return o, fixed_sum(np.sqrt(_sq3(step))) / g.n


def irls_weights(r, sigma):
    t = _sq3(r) + sigma * sigma
    return sigma / (t * t)


def l1_solve(g, solver, b, max_iterations, b_sq, margins):
    """L1Solver::Solve (math/l1_solver.h:120-178).  Returns (x, iterations run)."""
    z = np.zeros((g.E, 3))
    u = np.zeros((g.E, 3))
    x = np.zeros((g.n, 3))
    rhs_norm = np.sqrt(b_sq)
    primal_abs = np.sqrt(3.0 * g.E) * ABS_TOL
    dual_abs = np.sqrt(3.0 * g.n) * ABS_TOL
    ran = 0
    for _ in range(max_iterations):
        x = solver.solve(g.At(b + z - u))
        ax = g.A(x)
        ax_hat = ALPHA * ax
        ax_hat = ax_hat + (1.0 - ALPHA) * (z + b)
        z_old = z
        v = ax_hat - b + u
        kappa = 1.0 / RHO
        z = np.maximum(0.0, v - kappa) - np.maximum(0.0, -v - kappa)
        u = u + (ax_hat - z - b)
        r_norm = np.sqrt(fixed_sum(_sq3(ax - z - b)))
        s_norm = np.sqrt(fixed_sum(_sq3(-RHO * g.At(z - z_old))))
        max_norm = max(np.sqrt(fixed_sum(_sq3(ax))), np.sqrt(fixed_sum(_sq3(z))), rhs_norm)
        primal_eps = primal_abs + REL_TOL * max_norm
        dual_eps = dual_abs + REL_TOL * np.sqrt(fixed_sum(_sq3(RHO * g.At(u))))
        ran += 1
        margins.append(_margin(r_norm, primal_eps))
        margins.append(_margin(s_norm, dual_eps))
        if r_norm < primal_eps and s_norm < dual_eps:
            break
    return x, ran


def estimate(num_views, view1, view2, relative_rotations, orientations, fixed_view=0, options=None, lu=False, perm=None):
    """Returns a dict: rotations [V, 3], residuals [E, 3], admm_iterations, l1_steps, irls_steps, irls_sq_residuals,
    l1_converged, irls_converged, factorizations, margins (one per decision), min_margin."""
    opt = dict(DEFAULTS)
    opt.update(options or {})
    o = np.array(orientations, dtype=np.float64).reshape(-1, 3)
    rel = np.asarray(relative_rotations, dtype=np.float64).reshape(-1, 3)
    view1, view2 = np.asarray(view1), np.asarray(view2)
    if perm is not None:  # view v becomes view perm[v]
        perm = np.asarray(perm)
        back = np.empty_like(perm)
        back[perm] = np.arange(perm.size)
        res = estimate(num_views, perm[view1], perm[view2], rel, o[back], int(perm[fixed_view]), options, lu)
        res["rotations"] = res["rotations"][perm]
        return res
    g = Graph(num_views, view1, view2, fixed_view)
    margins, admm, l1_steps, irls_steps, irls_sq = [], [], [], [], []
    l1_converged = irls_converged = False
    factorizations = 0
    r = compute_residuals(g, rel, o)
    r_sq = fixed_sum(_sq3(r))
    if opt["max_num_l1_iterations"] > 0:
        solver = _Solver(g.laplacian(), lu)
        factorizations += 1
        budget = ADMM_FIRST_BUDGET
        for _ in range(opt["max_num_l1_iterations"]):
            step, ran = l1_solve(g, solver, r, budget, r_sq, margins)
            admm.append(ran)
            o, avg = update_rotations(g, o, step)
            r = compute_residuals(g, rel, o)
            r_sq = fixed_sum(_sq3(r))
            l1_steps.append(avg)
            margins.append(_margin(avg, opt["l1_step_convergence_threshold"]))
            if avg <= opt["l1_step_convergence_threshold"]:
                l1_converged = True
                break
            budget *= 2
    sigma = opt["irls_loss_parameter_sigma"]
    for _ in range(opt["max_num_irls_iterations"]):
        w = irls_weights(r, sigma)
        solver = _Solver(g.laplacian(w), lu)
        factorizations += 1
        step = solver.solve(g.At(w[:, None] * r))
        o, avg = update_rotations(g, o, step)
        r = compute_residuals(g, rel, o)
        r_sq = fixed_sum(_sq3(r))
        irls_steps.append(avg)
        irls_sq.append(r_sq)
        margins.append(_margin(avg, opt["irls_step_convergence_threshold"]))
        if avg < opt["irls_step_convergence_threshold"]:
            irls_converged = True
            break
    return dict(rotations=o, residuals=r, admm_iterations=admm, l1_steps=l1_steps, irls_steps=irls_steps,
                irls_sq_residuals=irls_sq, l1_converged=l1_converged, irls_converged=irls_converged,
                factorizations=factorizations, margins=margins, min_margin=min(margins) if margins else np.inf)


# ---- scenes and measures ----------------------------------------------------------------------------------------------
def relative_rotation(o1, o2, noise_deg, rng):
    """R_12 = N R(o2) R(o1)^T with N a rotation of noise_deg degrees about a random axis (the reference test's
    RelativeRotationFromTwoRotations, robust_rotation_estimator_test.cc:59-73)."""
    o1, o2 = np.atleast_2d(o1), np.atleast_2d(o2)
    axis = rng.uniform(-1.0, 1.0, size=o1.shape)
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    N = angle_axis_to_matrix(axis * np.deg2rad(noise_deg))
    R1, R2 = angle_axis_to_matrix(o1), angle_axis_to_matrix(o2)
    return matrix_to_angle_axis(matmul3(N, matmul3(R2, np.transpose(R1, (0, 2, 1)))))


def chain_initialisation(num_views, view1, view2, rel):
    """InitializeRotationsFromSpanningTree (:200-209): view 0 at the origin, view i from view i - 1 through edge
    (i - 1, i), which the scenes below put at edge index i - 1."""
    o = np.zeros((num_views, 3))
    for i in range(1, num_views):
        assert view1[i - 1] == i - 1 and view2[i - 1] == i
        o[i] = multiply_rotations(rel[i - 1], o[i - 1])[0]
    return o


def make_scene(num_views, num_pairs, noise_deg, seed, outlier_fraction=0.0, scale=0.2):
    """The reference test's scene (:159-197): orientations scale * uniform(-1, 1)^3, the chain (i - 1, i) first, then
    random distinct pairs with view1 < view2.  outlier_fraction of the non-chain edges get a random rotation instead.
    Returns (ground truth [V, 3], view1, view2, rel [E, 3], initial orientations [V, 3])."""
    rng = np.random.default_rng(seed)
    gt = scale * rng.uniform(-1.0, 1.0, size=(num_views, 3))
    pairs = [(i - 1, i) for i in range(1, num_views)]
    seen = set(pairs)
    assert num_pairs <= num_views * (num_views - 1) // 2
    while len(pairs) < num_pairs:
        a, b = (int(x) for x in rng.integers(0, num_views, size=2))
        if a > b:
            a, b = b, a
        if a == b or (a, b) in seen:
            continue
        seen.add((a, b))
        pairs.append((a, b))
    v1 = np.array([p[0] for p in pairs], dtype=np.int32)
    v2 = np.array([p[1] for p in pairs], dtype=np.int32)
    rel = relative_rotation(gt[v1], gt[v2], noise_deg, rng)
    n_out = int(round(outlier_fraction * num_pairs))
    if n_out:
        which = rng.choice(np.arange(num_views - 1, num_pairs), size=n_out, replace=False)
        axis = rng.normal(size=(n_out, 3))
        axis /= np.linalg.norm(axis, axis=1, keepdims=True)
        rel[which] = axis * rng.uniform(0.0, np.pi, size=(n_out, 1))
    return gt, v1, v2, rel, chain_initialisation(num_views, v1, v2, rel)


def rotation_angles(a, b):
    """The angle of R(a) R(b)^T per row, radians."""
    Ra, Rb = angle_axis_to_matrix(a), angle_axis_to_matrix(b)
    D = matmul3(Ra, np.transpose(Rb, (0, 2, 1)))
    sx, sy, sz = D[:, 2, 1] - D[:, 1, 2], D[:, 0, 2] - D[:, 2, 0], D[:, 1, 0] - D[:, 0, 1]
    return np.arctan2(0.5 * np.sqrt(sx * sx + sy * sy + sz * sz), 0.5 * (D[:, 0, 0] + D[:, 1, 1] + D[:, 2, 2] - 1.0))


def aligned_errors_deg(gt, est):
    """The angle between R(gt_i) and R(est_i) Q per view, in degrees, for the rotation Q that minimises the chordal
    distance sum_i |R(est_i) Q - R(gt_i)|_F^2: Q = U V^T of the SVD of sum_i R(est_i)^T R(gt_i), det +1."""
    Rg, Re = angle_axis_to_matrix(gt), angle_axis_to_matrix(est)
    M = np.einsum("nji,njk->ik", Re, Rg)
    U, _, Vt = np.linalg.svd(M)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    Q = U @ D @ Vt
    aligned = Re @ Q
    return np.rad2deg(rotation_angles(matrix_to_angle_axis(aligned), gt))


def model_spread(num_views, view1, view2, rel, o, fixed_view, options, base=None, seed=1):
    """The larger of two differences on the same input, each the largest of the per-view rotation angle and the
    per-edge residual difference: the model against its LU variant, and against its permuted-numbering variant."""
    base = base or estimate(num_views, view1, view2, rel, o, fixed_view, options)
    perm = np.random.default_rng(seed).permutation(num_views)
    spread = 0.0
    for other in (estimate(num_views, view1, view2, rel, o, fixed_view, options, lu=True),
                  estimate(num_views, view1, view2, rel, o, fixed_view, options, perm=perm)):
        spread = max(spread, float(rotation_angles(other["rotations"], base["rotations"]).max()),
                     float(np.abs(other["residuals"] - base["residuals"]).max()))
    return spread
