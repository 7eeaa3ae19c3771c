"""numpy restatement of theia::LeastUnsquaredDeviationPositionEstimator
(least_unsquared_deviation_position_estimator.cc:75-212, math/constrained_l1_solver.cc:49-187) in the fixed orders of
tmi_ba_estimate_global_positions_lud (include/theia_mi355_ba.h):

  * views are a dense table, `fixed_view` is at 0; free view v has columns 3 (v - (v > fixed_view)) + c, edge e has
    column 3 n + e, n = V - 1; rows 3 e + c are p[view2] - p[view1] - s_e t_e, rows 3 E + e are s_e, b = [0; 1];
  * with d_e = |t_e|^2 + 1 and W_e = I3 - t_e t_e^T / d_e the scales are eliminated: ONE symmetric positive definite
    matrix S of order 3 n (schur_matrix), factored once;
  * every per-view sum over a view's edges runs from zero in ascending edge index (np.add.at is unbuffered and applies
    its updates in the order given);
  * every norm is a reduction of fixed shape: blocks of 256 consecutive items are added by a binary tree, the block sums
    are dealt to 256 accumulators in ascending order and those are added by the same tree; for the two norms of A^T
    products the edges' block sums (the scale entries) come before the views' (the position entries).

Three solve paths exist to measure the model against itself: solve="schur" goes through S as the device does,
"cholesky" and "lu" factor the full A^T A of order 3 n + E built from A ENTRY BY ENTRY as the reference builds it
(constraint_matrix, :154-212 and constrained_l1_solver.cc:62-83); perm renumbers the views (the edges keep their order)
and maps the result back.  Every stopping decision is recorded with its margin, the relative distance
|norm - eps| / eps: for an iteration that stops the smaller of the two (either comparison failing would have gone on),
for one that does not the margin of the comparison that held it (the larger, when both did).
"""
import numpy as np

import robust_rotation_model as rot
from robust_rotation_model import _margin, _sq3, _tree256

# math/constrained_l1_solver.h:64-74; the estimator's own Options are only CHECKed (:67-73)
DEFAULTS = dict(max_num_iterations=1000, rho=10.0, alpha=1.2, absolute_tolerance=1e-4, relative_tolerance=1e-2)


def _dot3(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _block_parts(x):
    x = np.asarray(x, dtype=np.float64).ravel()
    nb = max((x.size + 255) // 256, 1)
    pad = np.zeros(nb * 256)
    pad[:x.size] = x
    return _tree256(pad.reshape(nb, 256))


def fixed_sum_parts(arrays):
    """The second stage of rot.fixed_sum over the block sums of several arrays laid side by side."""
    part = np.concatenate([_block_parts(a) for a in arrays])
    acc = np.zeros(256)
    for k in range(0, part.size, 256):
        chunk = part[k:k + 256]
        acc[:chunk.size] += chunk
    return float(_tree256(acc.reshape(1, 256))[0])


def directions(view_rotation, view1, position2):
    """t_e = R(view_rotation[view1])^T position_2 (:56-63); view_rotation None: position_2 as it is."""
    p = np.asarray(position2, dtype=np.float64).reshape(-1, 3)
    if view_rotation is None:
        return p.copy()
    R = rot.angle_axis_to_matrix(np.asarray(view_rotation, dtype=np.float64).reshape(-1, 3)[np.asarray(view1)])
    return np.stack([(R[:, 0, k] * p[:, 0] + R[:, 1, k] * p[:, 1]) + R[:, 2, k] * p[:, 2] for k in range(3)], axis=1)


def edge_blocks(t):
    """d_e [E] and W_e [E, 3, 3]"""
    d = _sq3(t) + 1.0
    W = np.eye(3)[None, :, :] - (t[:, :, None] * t[:, None, :]) / d[:, None, None]
    return d, W


def schur_matrix(g, t):
    """S [3 n, 3 n]: the diagonal block of a view is the sum of W_e over its edges in ascending edge index, block
    (view1, view2) of an edge minus the sum of W_e over the edges of that pair in ascending edge index."""
    _, W = edge_blocks(t)
    diag = np.zeros((g.V, 3, 3))
    np.add.at(diag, g.ends, np.repeat(W, 2, axis=0))
    diag = np.delete(diag, g.fixed, axis=0)
    off = np.zeros((g.n, g.n, 3, 3))
    both = (g.c1 >= 0) & (g.c2 >= 0)
    a, b, Wb = g.c1[both], g.c2[both], W[both]
    np.add.at(off, (np.stack([a, b], axis=1).ravel(), np.stack([b, a], axis=1).ravel()), np.repeat(Wb, 2, axis=0))
    blocks = -off
    blocks[np.arange(g.n), np.arange(g.n)] = diag
    return blocks.transpose(0, 2, 1, 3).reshape(3 * g.n, 3 * g.n)


def constraint_matrix(g, t):
    """A [4 E, 3 n + E] entry by entry as SetupConstraintMatrix (:154-212) and ConstrainedL1Solver (:62-80) write it."""
    E, n = g.E, g.n
    A = np.zeros((4 * E, 3 * n + E))
    for e in range(E):
        for c in range(3):
            if g.c1[e] >= 0:
                A[3 * e + c, 3 * g.c1[e] + c] = -1.0
            if g.c2[e] >= 0:
                A[3 * e + c, 3 * g.c2[e] + c] = 1.0
            A[3 * e + c, 3 * n + e] = -t[e, c]
        A[3 * E + e, 3 * n + e] = 1.0
    return A


def _admm_rows(ax, b, l1, alpha, kappa, z, u):
    """One block of rows of :141-150.  Returns (z, u, z - z_old, A x - z - b)."""
    ax_hat = alpha * ax
    ax_hat = ax_hat + (1.0 - alpha) * (z + b)
    v = (ax_hat - b) + u
    znew = np.maximum(0.0, v - kappa) - np.maximum(0.0, -v - kappa) if l1 else np.maximum(v, 0.0)
    return znew, u + ((ax_hat - znew) - b), znew - z, (ax - znew) - b


def estimate(num_views, view1, view2, position2, view_rotation=None, fixed_view=0, options=None, solve="schur",
             perm=None):
    """Returns a dict: positions [V, 3] (the fixed view at 0), scales [E], residuals [E, 3] (the final A x of the L1
    rows), r_norms, s_norms, iterations, converged, margins (one per iteration), min_margin."""
    opt = dict(DEFAULTS)
    opt.update(options or {})
    view1, view2 = np.asarray(view1), np.asarray(view2)
    if perm is not None:  # view v becomes view perm[v]
        perm = np.asarray(perm)
        back = np.empty_like(perm)
        back[perm] = np.arange(perm.size)
        vr = None if view_rotation is None else np.asarray(view_rotation, dtype=np.float64).reshape(-1, 3)[back]
        res = estimate(num_views, perm[view1], perm[view2], position2, vr, int(perm[fixed_view]), options, solve)
        res["positions"] = res["positions"][perm]
        return res
    g = rot.Graph(num_views, view1, view2, fixed_view)
    E, n = g.E, g.n
    rho, alpha = opt["rho"], opt["alpha"]
    kappa = 1.0 / rho
    t = directions(view_rotation, view1, position2)
    d, _ = edge_blocks(t)
    if solve == "schur":
        solver = rot._Solver(schur_matrix(g, t), False)
    else:
        A = constraint_matrix(g, t)
        solver = rot._Solver(A.T @ A, solve == "lu")
    z_l, u_l, dz_l = np.zeros((E, 3)), np.zeros((E, 3)), np.zeros((E, 3))
    z_s, u_s = np.zeros(E), np.zeros(E)
    qs = np.ones(E)  # the scale entries of A^T b
    rhs_norm = np.sqrt(float(E))
    primal_abs = np.sqrt(4.0 * E) * opt["absolute_tolerance"]
    dual_abs = np.sqrt(3.0 * n + E) * opt["absolute_tolerance"]
    margins, r_norms, s_norms = [], [], []
    converged = False
    p, s, ax_l = np.zeros((n, 3)), np.zeros(E), np.zeros((E, 3))
    for _ in range(opt["max_num_iterations"]):
        q_p = g.At((0.0 + z_l) - u_l)
        if solve == "schur":
            rhs = q_p + g.At(t * (qs / d)[:, None])
            p = solver.solve(rhs.ravel()).reshape(n, 3)
            dp = g.A(p)
            s = (qs + _dot3(t, dp)) / d
        else:
            x = solver.solve(np.concatenate([q_p.ravel(), qs]))
            p, s = x[:3 * n].reshape(n, 3), x[3 * n:]
            dp = g.A(p)
        ax_l = dp - s[:, None] * t
        z_l, u_l, dz_l, res_l = _admm_rows(ax_l, 0.0, True, alpha, kappa, z_l, u_l)
        z_s, u_s, dz_s, res_s = _admm_rows(s, 1.0, False, alpha, kappa, z_s, u_s)
        qs = ((1.0 + z_s) - u_s) - _dot3(t, (0.0 + z_l) - u_l)
        sd = -rho * (dz_s - _dot3(t, dz_l))
        su = rho * (u_s - _dot3(t, u_l))
        r_norm = np.sqrt(rot.fixed_sum(_sq3(res_l) + res_s * res_s))
        ax_norm = np.sqrt(rot.fixed_sum(_sq3(ax_l) + s * s))
        z_norm = np.sqrt(rot.fixed_sum(_sq3(z_l) + z_s * z_s))
        s_norm = np.sqrt(fixed_sum_parts([sd * sd, _sq3(-rho * g.At(dz_l))]))
        t_norm = np.sqrt(fixed_sum_parts([su * su, _sq3(rho * g.At(u_l))]))
        primal_eps = primal_abs + opt["relative_tolerance"] * max(ax_norm, z_norm, rhs_norm)
        dual_eps = dual_abs + opt["relative_tolerance"] * t_norm
        r_norms.append(r_norm)
        s_norms.append(s_norm)
        mr, ms = _margin(r_norm, primal_eps), _margin(s_norm, dual_eps)
        r_ok, s_ok = r_norm < primal_eps, s_norm < dual_eps
        if r_ok and s_ok:
            margins.append(min(mr, ms))
            converged = True
            break
        margins.append(max(mr, ms) if not (r_ok or s_ok) else (ms if r_ok else mr))
    positions = np.insert(p, g.fixed, 0.0, axis=0)
    return dict(positions=positions, scales=s, residuals=ax_l, r_norms=np.array(r_norms), s_norms=np.array(s_norms),
                iterations=len(r_norms), converged=converged, margins=margins, min_margin=min(margins))


# ---- scenes and measures ----------------------------------------------------------------------------------------------
def relative_directions(orientations, positions, view1, view2, noise_deg, rng):
    """position_2 of every pair as the reference test's CreateTwoViewInfo makes it (..._test.cc:82-93, :187-211):
    N R(orientation1) (c2 - c1) / |c2 - c1| with N a rotation by noise_deg * uniform(-1, 1) degrees about a random
    axis."""
    E = len(view1)
    noise = noise_deg * rng.uniform(-1.0, 1.0, size=(E, 2))  # ([:, 0] is the rotation's in the reference)
    axis = rng.uniform(-1.0, 1.0, size=(E, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    N = rot.angle_axis_to_matrix(axis * np.deg2rad(noise[:, 1])[:, None])
    R1 = rot.angle_axis_to_matrix(orientations[view1])
    u = positions[view2] - positions[view1]
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return np.einsum("eij,ejk,ek->ei", N, R1, u)


def random_pairs(num_views, num_pairs, rng):
    """The chain (i - 1, i) first, then random distinct pairs with view1 < view2 (..._test.cc:164-185)."""
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
    return pairs


def scene_on_pairs(num_views, pairs, noise_deg, seed, outlier_fraction=0.0):
    """Orientations 0.2 uniform(-1, 1)^3 and positions 10 uniform(-1, 1)^3 (..._test.cc:155-162) on the given pairs
    (either direction).  outlier_fraction of the edges after the first num_views - 1 get a random unit direction.
    Returns (ground-truth positions [V, 3], orientations [V, 3], view1, view2, position_2 [E, 3])."""
    rng = np.random.default_rng(seed)
    orientations = 0.2 * rng.uniform(-1.0, 1.0, size=(num_views, 3))
    positions = 10.0 * rng.uniform(-1.0, 1.0, size=(num_views, 3))
    v1 = np.array([p[0] for p in pairs], dtype=np.int32)
    v2 = np.array([p[1] for p in pairs], dtype=np.int32)
    pos2 = relative_directions(orientations, positions, v1, v2, noise_deg, rng)
    n_out = int(round(outlier_fraction * (len(pairs) - (num_views - 1))))
    if n_out:
        which = rng.choice(np.arange(num_views - 1, len(pairs)), size=n_out, replace=False)
        bad = rng.normal(size=(n_out, 3))
        pos2[which] = bad / np.linalg.norm(bad, axis=1, keepdims=True)
    return positions, orientations, v1, v2, pos2


def make_scene(num_views, num_pairs, noise_deg, seed, outlier_fraction=0.0):
    """The reference test's scene; the pairs are drawn from their own stream so that they do not depend on the noise."""
    pairs = random_pairs(num_views, num_pairs, np.random.default_rng([seed, 1]))
    return scene_on_pairs(num_views, pairs, noise_deg, seed, outlier_fraction)


def aligned_errors(gt, est):
    """|gt_i - (c R est_i + t)| per view for the similarity of Umeyama (1991) that takes est to gt, as the reference
    test's AlignPositions (..._test.cc:97-116)."""
    mu_e, mu_g = est.mean(axis=0), gt.mean(axis=0)
    de, dg = est - mu_e, gt - mu_g
    U, D, Vt = np.linalg.svd(dg.T @ de / est.shape[0])
    Sg = np.diag([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
    R = U @ Sg @ Vt
    c = np.trace(np.diag(D) @ Sg) / (de * de).sum() * est.shape[0]
    return np.linalg.norm(gt - (c * (est @ R.T) + (mu_g - c * R @ mu_e)), axis=1)


def difference(a, b, scale):
    """max |a - b| over positions and scales, over `scale`"""
    return max(float(np.abs(a["positions"] - b["positions"]).max()), float(np.abs(a["scales"] - b["scales"]).max())) / scale


def model_spread(num_views, view1, view2, position2, view_rotation, fixed_view, options, base=None, seed=1):
    """The largest difference (positions and scales, over the largest |position| of the base) of the model from its
    full-Cholesky variant, its LU variant and its permuted-numbering variant on the same input."""
    args = (num_views, view1, view2, position2, view_rotation, fixed_view, options)
    base = base or estimate(*args)
    scale = float(np.abs(base["positions"]).max())
    perm = np.random.default_rng(seed).permutation(num_views)
    return max(difference(estimate(*args, solve="cholesky"), base, scale),
               difference(estimate(*args, solve="lu"), base, scale),
               difference(estimate(*args, perm=perm), base, scale))
