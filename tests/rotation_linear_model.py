"""A numpy restatement of tmi_ba_estimate_global_rotations_linear (theiasfm_amd/csrc/rotation_linear_kernels.h and its
host loop in pose_graph_calls.h), step for step: the matrix M of linear_rotation_estimator.cc:90-152, the start block from the
splitmix64 stream, the factorisation of M + mu I, subspace iteration on six columns with two passes of modified
Gram-Schmidt on unnormalised dots, Rayleigh-Ritz by cyclic Jacobi with the device's sweep order, ordering and sign rule,
the stop rule, and the projection by a one-sided Jacobi SVD.  The factorisation and the sums are numpy's, so the device
agrees with this model to rounding amplified by the problem's conditioning, not bit for bit.

`plain` is the answer without any of that: the dense M, numpy.linalg.eigh, the three smallest eigenvectors, the same
projection.

Both return rotations that are defined up to one rotation applied on the right of every view: compare loop
rotations (`loop_angles`), or align first (`aligned_angles`)."""
import numpy as np

from rotation_nonlinear_model import loop_rotations, matrices_to_angle_axis, rotation_matrices  # noqa: F401

BLOCK = 6
JACOBI_SWEEPS = 12
SVD_SWEEPS = 12
EPS = 2.220446049250313e-16
DEFAULTS = dict(max_iterations=1000, tolerance=1e-10, relative_shift=1e-9, seed=0)
_MASK = (1 << 64) - 1


def splitmix64_words(seed, count):
    """Words 0 .. count-1 of the splitmix64 stream from state `seed` (ransac_core.h: splitmix64_word)."""
    c = np.arange(1, count + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed & _MASK) + c * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def start_block(n, seed):
    """Q [n, 6]: Q[i, j] = 2 u - 1, u = ((word >> 11) + 0.5) 2^-53, word 6 i + j."""
    w = splitmix64_words(seed, n * BLOCK)
    u = ((w >> np.uint64(11)).astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)
    return (2.0 * u - 1.0).reshape(n, BLOCK)


def problem(num_views, view1, view2):
    """The views with an edge in ascending index, the edges on those, the degrees."""
    view1, view2 = np.asarray(view1, dtype=np.int64), np.asarray(view2, dtype=np.int64)
    views = np.unique(np.concatenate([view1, view2]))
    index = np.full(num_views, -1, dtype=np.int64)
    index[views] = np.arange(views.size)
    a, b = index[view1], index[view2]
    degree = np.bincount(np.concatenate([a, b]), minlength=views.size)
    return views, a, b, degree


def assemble(a, b, rel, num_problem_views):
    """M of order 3 Vp: the degree on the diagonal, -R12^T at block (view1, view2), -R12 at block (view2, view1)."""
    n = 3 * num_problem_views
    M = np.zeros((n, n))
    R = rotation_matrices(rel)
    for e in range(a.size):
        i, j = 3 * a[e], 3 * b[e]
        M[i:i + 3, j:j + 3] = -R[e].T
        M[j:j + 3, i:i + 3] = -R[e]
        M[i:i + 3, i:i + 3] += np.eye(3)
        M[j:j + 3, j:j + 3] += np.eye(3)
    return M


def mgs_pass(Y):
    """One pass of the device's Gram-Schmidt: step j takes s_jk = y_j . y_k (k >= j) on the unnormalised column, then
    q_j = y_j / sqrt(s_jj) and y_k -= (s_jk / sqrt(s_jj)) q_j; a column that vanished stays zero."""
    Y = Y.copy()
    for j in range(BLOCK):
        s = Y[:, j] @ Y[:, j:]
        inv = 1.0 / np.sqrt(s[0]) if s[0] > 0.0 else 0.0
        q = Y[:, j] * inv
        Y[:, j] = q
        for k in range(j + 1, BLOCK):
            Y[:, k] -= (s[k - j] * inv) * q
    return Y


def jacobi6(T):
    """Cyclic Jacobi on the symmetric 6 x 6 T as lin_ritz_kernel runs it.  Returns (theta ascending, W with column j
    the j-th Ritz vector, signed, and the sign rule's margin over the first three columns)."""
    A = np.array(np.triu(T) + np.triu(T, 1).T, dtype=np.float64)
    W = np.eye(BLOCK)
    for _ in range(JACOBI_SWEEPS):
        for p in range(BLOCK - 1):
            for q in range(p + 1, BLOCK):
                apq = A[p, q]
                if apq == 0.0:
                    continue
                with np.errstate(over="ignore"):  # (a tiny a_pq: zeta is infinite and t = 0, as on the device)
                    zeta = (A[q, q] - A[p, p]) / (2.0 * apq)
                    t = (1.0 if zeta >= 0.0 else -1.0) / (abs(zeta) + np.sqrt(zeta * zeta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                cp, cq = A[:, p].copy(), A[:, q].copy()
                A[:, p], A[:, q] = c * cp - s * cq, s * cp + c * cq
                rp, rq = A[p, :].copy(), A[q, :].copy()
                A[p, :], A[q, :] = c * rp - s * rq, s * rp + c * rq
                wp, wq = W[:, p].copy(), W[:, q].copy()
                W[:, p], W[:, q] = c * wp - s * wq, s * wp + c * wq
    d = np.diag(A)
    order = np.argsort(d, kind="stable")  # ascending, the first of equals first
    theta = d[order]
    Ws = W[:, order].copy()
    margin = np.inf
    for j in range(BLOCK):
        mag = np.abs(Ws[:, j])
        k = int(np.argmax(mag))  # the first of equals
        if Ws[k, j] < 0.0:
            Ws[:, j] = -Ws[:, j]
        if j < 3:
            rest = np.delete(mag, k)
            margin = min(margin, float((mag[k] - rest.max()) / mag[k]))
    return theta, Ws, margin


def project(B):
    """[V, 3, 3] blocks to SO(3) as lin_project_kernel does: U V^T by one-sided Jacobi, negated where det < 0.  Returns
    (R [V, 3, 3], negated [V] bool)."""
    A = np.array(B, dtype=np.float64).transpose(0, 2, 1).copy()  # A[:, c] = column c
    Vm = np.broadcast_to(np.eye(3), A.shape).copy()
    for _ in range(SVD_SWEEPS):
        for p, q in ((0, 1), (0, 2), (1, 2)):
            alpha = (A[:, p] ** 2).sum(axis=1)
            beta = (A[:, q] ** 2).sum(axis=1)
            gamma = (A[:, p] * A[:, q]).sum(axis=1)
            live = gamma != 0.0
            g = np.where(live, gamma, 1.0)
            zeta = (beta - alpha) / (2.0 * g)
            t = np.where(zeta >= 0.0, 1.0, -1.0) / (np.abs(zeta) + np.sqrt(zeta * zeta + 1.0))
            c = np.where(live, 1.0 / np.sqrt(t * t + 1.0), 1.0)
            s = np.where(live, t * c, 0.0)
            for X in (A, Vm):
                xp, xq = X[:, p].copy(), X[:, q].copy()
                X[:, p] = c[:, None] * xp - s[:, None] * xq
                X[:, q] = s[:, None] * xp + c[:, None] * xq
    sigma = np.sqrt((A ** 2).sum(axis=2))
    U = A * np.where(sigma > 0.0, 1.0 / np.where(sigma > 0.0, sigma, 1.0), 0.0)[:, :, None]
    for c in range(3):
        a, b = (c + 1) % 3, (c + 2) % 3
        fix = ~(sigma[:, c] > 0.0) & (sigma[:, a] > 0.0) & (sigma[:, b] > 0.0)
        U[fix, c] = np.cross(U[fix, a], U[fix, b])
    R = np.einsum("vkr,vkc->vrc", U, Vm)
    negated = np.linalg.det(R) < 0.0
    R[negated] = -R[negated]
    return R, negated


def _blocks(Q):
    return Q[:, :3].reshape(-1, 3, 3)


def estimate(num_views, view1, view2, rel, options=None, view_rotation=None):
    """The device call.  Returns a dict: rotations [V, 3] (views without an edge as given, default 0), num_views,
    num_pairs, order, iterations, converged, usable, eigenvalue [4], residual [3], num_reflected, max_degree,
    stop_margin (|largest residual - threshold| / threshold, the smaller of the last two iterations) and sign_margin
    (the smallest, over the iterations, of the sign rule's margin and of the gaps between the first four Ritz values
    relative to 2 x the largest degree)."""
    o = dict(DEFAULTS)
    o.update(options or {})
    rel = np.asarray(rel, dtype=np.float64).reshape(-1, 3)
    views, a, b, degree = problem(num_views, view1, view2)
    Vp, n = views.size, 3 * views.size
    maxdeg = int(degree.max())
    out = dict(rotations=np.zeros((num_views, 3)) if view_rotation is None else np.array(view_rotation, dtype=np.float64),
               num_views=Vp, num_pairs=int(a.size), order=n, iterations=0, converged=0, usable=0, num_reflected=0,
               eigenvalue=np.zeros(4), residual=np.zeros(3), max_degree=maxdeg, stop_margin=np.inf, sign_margin=np.inf)
    M = assemble(a, b, rel, Vp)
    mu = o["relative_shift"] * maxdeg
    try:
        L = np.linalg.cholesky(M + mu * np.eye(n))
    except np.linalg.LinAlgError:
        return out
    out["usable"] = 1
    threshold = o["tolerance"] * 2.0 * maxdeg
    Q = start_block(n, o["seed"])
    margins = []
    while out["iterations"] < o["max_iterations"] and not out["converged"]:
        out["iterations"] += 1
        Y = np.linalg.solve(L.T, np.linalg.solve(L, Q))
        Y = mgs_pass(mgs_pass(Y))
        Z = M @ Y
        theta, W, sign_margin = jacobi6(Y.T @ Z)
        Q, Z = Y @ W, Z @ W
        res = np.sqrt(((Z[:, :3] - theta[:3] * Q[:, :3]) ** 2).sum(axis=0))
        out["converged"] = int(bool((res <= threshold).all()))
        margins.append(abs(float(res.max()) - threshold) / threshold)
        gap = float(np.diff(theta[:4]).min()) / (2.0 * maxdeg)
        out["sign_margin"] = min(out["sign_margin"], sign_margin, gap)
    out["eigenvalue"], out["residual"] = theta[:4].copy(), res
    out["stop_margin"] = min(margins[-2:])
    R, negated = project(_blocks(Q))
    out["rotations"][views] = matrices_to_angle_axis(R)
    out["num_reflected"] = int(negated.sum())
    out["vectors"] = Q[:, :3].copy()
    return out


def plain(num_views, view1, view2, rel):
    """Dense M, numpy.linalg.eigh, the three smallest eigenvectors, the same projection.  Returns a dict: rotations
    [V, 3], eigenvalues (all, ascending), num_reflected, max_degree."""
    rel = np.asarray(rel, dtype=np.float64).reshape(-1, 3)
    views, a, b, degree = problem(num_views, view1, view2)
    w, X = np.linalg.eigh(assemble(a, b, rel, views.size))
    R, negated = project(_blocks(X))
    rotations = np.zeros((num_views, 3))
    rotations[views] = matrices_to_angle_axis(R)
    return dict(rotations=rotations, eigenvalues=w, num_reflected=int(negated.sum()), max_degree=int(degree.max()))


# ---- comparisons ---------------------------------------------------------------------------------------------------------
def _angles(D):
    """The rotation angles of the [N, 3, 3] rotations D (radians), accurate near zero."""
    return 2.0 * np.arcsin(np.minimum(np.linalg.norm(D - np.eye(3), axis=(1, 2)) / (2.0 * np.sqrt(2.0)), 1.0))


def loop_angles(x, y, view1, view2):
    """Per pair the angle between the loop rotations R_j R_i^T of the results x and y ([V, 3] angle-axis)."""
    Lx, Ly = loop_rotations(x, view1, view2), loop_rotations(y, view1, view2)
    return _angles(Lx @ Ly.transpose(0, 2, 1))


def aligned_angles(x, gt, views):
    """Per view the angle between R_x G and R_gt, G the one rotation that best maps x onto gt."""
    Rx, Rg = rotation_matrices(x)[views], rotation_matrices(gt)[views]
    U, _, Vt = np.linalg.svd(np.einsum("vji,vjk->ik", Rx, Rg))
    G = U @ np.diag([1.0, 1.0, np.linalg.det(U @ Vt)]) @ Vt
    return _angles((Rx @ G) @ Rg.transpose(0, 2, 1))


def derived_bound(c, num_problem_views, max_degree, tolerance, gap):
    """max(1e-9, c sqrt(V) (sqrt(3) tolerance 2 maxdeg + n eps 2 maxdeg) / (lambda_4 - lambda_3)) radians: Davis-Kahan
    for the subspace of three residuals at the stop rule plus the rounding of a product with M, sqrt(V) for a block of
    norm about 1 / sqrt(V), c for the projection and the two views of a loop."""
    n = 3 * num_problem_views
    numerator = np.sqrt(3.0) * tolerance * 2.0 * max_degree + n * EPS * 2.0 * max_degree
    return max(1e-9, c * np.sqrt(num_problem_views) * numerator / gap)
