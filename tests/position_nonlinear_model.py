"""numpy restatement of theia::NonlinearPositionEstimator (nonlinear_position_estimator.cc:86-214,
pairwise_translation_error.h:63-88) under Ceres 1.14's HuberLoss, Corrector, TrustRegionMinimizer and
LevenbergMarquardtStrategy, in the fixed orders of tmi_ba_estimate_global_positions_nonlinear
(include/theia_mi355_ba.h).  Written from the reference's functor and Ceres' rules:

  * views are a dense table, `fixed_view` is at 0 and constant; free view v has columns 3 (v - (v > fixed_view)) + k;
  * per edge d = p[view2] - p[view1], norm = sqrt((d0 d0 + d1 d1) + d2 d2) (1 where below 1e-12), r = d / norm - t_e;
    the Jacobian with respect to p[view2] is (I - u u^T) / norm, I on the small-norm branch, and its negative with
    respect to p[view1] (`jacobian_complex_step` differentiates the reference's formula to check that);
  * the corrector: sqrt(rho') on both where s = 0 or rho'' <= 0, Triggs' alpha otherwise;
  * the normal equations J~^T J~ y = J~^T r~ of order 3 n, block by block, every per-view sum from zero in ascending edge
    index (np.add.at is unbuffered and applies its updates in the order given), Jacobi scaling from the first
    linearisation, the LM diagonal clamp(A_ii, lo, hi) / radius, numpy.linalg.cholesky for the solve;
  * every scalar by the reduction of fixed shape of the rotation and LUD models (rot.fixed_sum).

Every decision of the loop is recorded with its margin, the relative distance of the compared value from its threshold.
"""
import numpy as np

import position_lud_model as lud
import robust_rotation_model as rot
from position_lud_model import aligned_errors, directions, make_scene, scene_on_pairs  # noqa: F401  (for the tests)
from robust_rotation_model import _margin, _sq3

# nonlinear_position_estimator.h:70-72 and ceres::Solver::Options
DEFAULTS = dict(max_num_iterations=400, robust_loss_width=0.1, seed=0, jacobi_scaling=1,
                max_num_consecutive_invalid_steps=5, function_tolerance=1e-6, gradient_tolerance=1e-10,
                parameter_tolerance=1e-8, initial_trust_region_radius=1e4, max_trust_region_radius=1e16,
                min_trust_region_radius=1e-32, min_relative_decrease=1e-3, min_lm_diagonal=1e-6, max_lm_diagonal=1e32)
DBL_MIN = 2.2250738585072014e-308
MASK = (1 << 64) - 1
# the planes of the symmetric 3 x 3 blocks: 00 01 02 11 12 22
PLANE = np.array([[0, 1, 2], [1, 3, 4], [2, 4, 5]])


def splitmix64_word(seed, c):
    """Word c of the splitmix64 stream from state `seed` (Steele, Lea and Flood 2014)."""
    z = (seed + (c + 1) * 0x9e3779b97f4a7c15) & MASK
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & MASK
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & MASK
    return z ^ (z >> 31)


def start_positions(num_views, seed, fixed_view):
    """Component k of view v: 100 (2 u - 1), u = ((word >> 11) + 0.5) 2^-53, word 3 v + k of the stream; the fixed view 0."""
    out = np.empty((num_views, 3))
    for v in range(num_views):
        for k in range(3):
            u = (float(splitmix64_word(seed, 3 * v + k) >> 11) + 0.5) * (1.0 / 9007199254740992.0)
            out[v, k] = 100.0 * (2.0 * u - 1.0)
    out[fixed_view] = 0.0
    return out


def huber(s, a):
    """ceres::HuberLoss::Evaluate: rho, rho', rho'' per item."""
    b = a * a
    outer = s > b
    r = np.sqrt(np.where(outer, s, 1.0))
    rho1 = np.where(outer, np.maximum(DBL_MIN, a / r), 1.0)
    rho0 = np.where(outer, 2.0 * a * r - b, s)
    rho2 = np.where(outer, -rho1 / (2.0 * np.where(outer, s, 1.0)), 0.0)
    return rho0, rho1, rho2, outer


def residuals(p1, p2, t):
    """The reference's functor on arrays [E, 3] (real or complex): r, u, norm, small."""
    d = p2 - p1
    norm = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    small = norm.real < 1e-12
    norm = np.where(small, 1.0, norm)
    u = d / norm[:, None]
    return u - t, u, norm, small


def jacobian_analytic(p1, p2, t):
    """dr / dp2 [E, 3, 3]: (I - u u^T) / norm, I on the small-norm branch."""
    _, u, norm, small = residuals(p1, p2, t)
    J = (np.eye(3)[None] - u[:, :, None] * u[:, None, :]) / norm[:, None, None]
    J[small] = np.eye(3)
    return J


def jacobian_complex_step(p1, p2, t, which=2, h=1e-30):
    """dr / dp(which) [E, 3, 3] by the complex step on the reference's formula (exact to rounding: no subtraction)."""
    J = np.empty((p1.shape[0], 3, 3))
    for k in range(3):
        a, b = p1.astype(complex), p2.astype(complex)
        (b if which == 2 else a)[:, k] += 1j * h
        J[:, :, k] = residuals(a, b, t.astype(complex))[0].imag / h
    return J


def corrected(r, J, width):
    """Ceres' Corrector (corrector.cc) on residuals [E, 3] and Jacobians [E, 3, 3]: (rho, r~, J~, outer).  Where
    s = 0 or rho'' <= 0 it scales both by sqrt(rho'); HuberLoss has rho'' <= 0 everywhere (asserted), so the alpha of
    the other case never arises."""
    s = _sq3(r)
    rho0, rho1, rho2, outer = huber(s, width)
    assert (rho2 <= 0.0).all()
    sqrt_rho1 = np.sqrt(rho1)
    return rho0, sqrt_rho1[:, None] * r, sqrt_rho1[:, None, None] * J, outer


def linearize(g, x, t, width):
    """At x [n, 3]: cost, r [E, 3], B [E, 3, 3] = J~^T J~, q [E, 3] = J~^T r~, and which branches the edges took."""
    full = np.insert(x, g.fixed, 0.0, axis=0)
    p1, p2 = full[g.v1], full[g.v2]
    r, _, _, small = residuals(p1, p2, t)
    rho0, rt, Jt, outer = corrected(r, jacobian_analytic(p1, p2, t), width)
    B = (Jt[:, 0, :, None] * Jt[:, 0, None, :] + Jt[:, 1, :, None] * Jt[:, 1, None, :]) + Jt[:, 2, :, None] * Jt[:, 2, None, :]
    q = (Jt[:, 0, :] * rt[:, 0, None] + Jt[:, 1, :] * rt[:, 1, None]) + Jt[:, 2, :] * rt[:, 2, None]
    return rot.fixed_sum(0.5 * rho0), r, B, q, small, outer


def cost_at(g, x, t, width):
    full = np.insert(x, g.fixed, 0.0, axis=0)
    r = residuals(full[g.v1], full[g.v2], t)[0]
    return rot.fixed_sum(0.5 * huber(_sq3(r), width)[0])


def normal_equations(g, B, q, scale):
    """The scaled normal matrix [3 n, 3 n] (both triangles), the scaled gradient and the unscaled one ([n, 3])."""
    diag = np.zeros((g.V, 3, 3))
    np.add.at(diag, g.ends, np.repeat(B, 2, axis=0))
    diag = np.delete(diag, g.fixed, axis=0)
    blocks = np.zeros((g.n, g.n, 3, 3))
    both = (g.c1 >= 0) & (g.c2 >= 0)
    a, b, Bb = g.c1[both], g.c2[both], B[both]
    blocks[a, b] = -Bb  # (no unordered pair appears twice)
    blocks[b, a] = -Bb
    blocks[np.arange(g.n), np.arange(g.n)] = diag
    A = blocks.transpose(0, 2, 1, 3).reshape(3 * g.n, 3 * g.n)
    s = scale.ravel()
    A = (A * s[:, None]) * s[None, :]
    grad = g.At(q)
    return A, grad * scale, grad


def estimate(num_views, view1, view2, position2, view_rotation=None, fixed_view=0, options=None, start=None):
    """Returns a dict: positions, initial_positions [V, 3], residuals [E, 3], costs, radii, outcomes (entry 0 the start,
    then one per iteration run: 1 accepted, 0 rejected, -1 invalid, 2 / 3 ended by the parameter / function tolerance),
    iterations, termination (0 CONVERGENCE, 1 NO_CONVERGENCE, 2 FAILURE), factorizations, margins, min_margin, and the
    branches seen: small_norm, outer, inner (any edge of any linearisation)."""
    opt = dict(DEFAULTS)
    opt.update(options or {})
    opt.pop("positions_given", None)
    g = rot.Graph(num_views, np.asarray(view1), np.asarray(view2), fixed_view)
    n, width = g.n, opt["robust_loss_width"]
    t = directions(view_rotation, view1, position2)
    initial = start_positions(num_views, opt["seed"], fixed_view) if start is None else np.array(start, dtype=np.float64)
    initial[fixed_view] = 0.0
    x = np.delete(initial, fixed_view, axis=0)
    seen = dict(small_norm=False, outer=False, inner=False)

    def lin(x):
        cost, r, B, q, small, outer = linearize(g, x, t, width)
        seen["small_norm"] |= bool(small.any())
        seen["outer"] |= bool(outer.any())
        seen["inner"] |= bool((~outer).any())
        return cost, r, B, q

    cost, r, B, q = lin(x)
    scale = np.ones((n, 3))
    if opt["jacobi_scaling"]:
        d = np.zeros((g.V, 3))
        np.add.at(d, g.ends, np.repeat(B[:, [0, 1, 2], [0, 1, 2]], 2, axis=0))
        scale = 1.0 / (1.0 + np.sqrt(np.delete(d, fixed_view, axis=0)))
    A, grad, grad_unscaled = normal_equations(g, B, q, scale)
    x_norm = np.sqrt(rot.fixed_sum(x.ravel() * x.ravel()))
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
            y = rot._Solver(damped, False).solve(grad.ravel()).reshape(n, 3)
        except np.linalg.LinAlgError:
            usable, y = False, np.zeros((n, 3))
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
        sd = g.A(step)
        Bs = (B[:, :, 0] * sd[:, 0, None] + B[:, :, 1] * sd[:, 1, None]) + B[:, :, 2] * sd[:, 2, None]
        mcc_edges = -(lud._dot3(sd, q) + 0.5 * lud._dot3(sd, Bs))
        mcc = rot.fixed_sum(mcc_edges)
        cand_cost = cost_at(g, cand, t, width)
        step_sq = rot.fixed_sum(step.ravel() * step.ravel())
        cand_x_sq = rot.fixed_sum(cand.ravel() * cand.ravel())
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
            lin_cost, r, B, q = lin(x)
            assert lin_cost == cost
            A, grad, grad_unscaled = normal_equations(g, B, q, scale)
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
    return dict(positions=np.insert(x, fixed_view, 0.0, axis=0), initial_positions=initial, residuals=r,
                costs=np.array(costs), radii=np.array(radii), outcomes=np.array(outcomes, dtype=np.int32), iterations=it,
                termination=termination, factorizations=factorizations, margins=margins,
                min_margin=min(margins) if margins else np.inf, **seen)
