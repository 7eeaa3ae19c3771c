"""Seeded synthetic bundle-adjustment problems at the BASELINE.json sizes.

No BAL / 1DSfM file exists in the container, so the benchmark and
the parity tests run on synthetic reconstructions with the named camera /
track / observation counts.  The scene is generated directly in the
reference's conventions:

  * camera = [position C(3), angle-axis w(3)] with q = R(w) (X - C)
    (reference: src/theia/sfm/camera/reprojection_error.h:62-83, camera.h:195-200),
    the camera looks along +z of its own frame;
  * PINHOLE intrinsics [f, ar, skew, px, py, k1, k2] (pinhole_camera_model.h:86-94),
    BAL-like: own intrinsics group per view, principal point (0, 0)
    (Bundler/BAL -> Theia convention);
  * homogeneous points with w = 1 (track.h:66-67).

Config 1 follows the recipe of the reference's own synthetic test scenes
(sfm/global_pose_estimation/nonlinear_position_estimator_test.cc:66-74,166-200):
positions 10*U(-1,1)^3, angle-axis 0.2*U(-1,1)^3, f = 800, pp = (500, 500),
points U(-1,1)^3 + (0,0,20), every view observes every track.

The larger configs are a "landmark" scene: cameras on a jittered ring looking
at a ball of points; each track is seen by k cameras drawn from a window of
the ring (k - 2 ~ Geometric so that mean k = N_obs / N_pts, window width
heavy-tailed), which gives a banded-plus-tail co-visibility structure whose
reduced camera matrix fill is controlled by ``spread``.
"""
from __future__ import annotations

import numpy as np
from scipy.spatial.transform import Rotation

from . import abi
from .abi import Problem

# (cameras, points, observations) of BASELINE.json configs[0..3]
CONFIG_SIZES = {
    "tiny": (3, 100, 300),
    "ladybug49": (49, 7776, 31843),
    "alamo": (570, 140000, 900000),
    "venice1778": (1778, 993923, 5001946),
    # the same sizes with 0.2 % of the tracks seen by 24..400 views (not a BASELINE config: a stress
    # case for the long-track paths, cf. SURVEY 8d "max k a few hundred")
    "venice1778_heavy": (1778, 993923, 5001946),
    # the same sizes with SEQUENCE structure (scene "street"): S is a band of ~10 % fill, PCG needs tens of
    # iterations per LM iteration -- what real collections look like, where the ring scene is a turntable
    "venice1778_street": (1778, 993923, 5001946),
}


# ---- numpy projection (generator side only) ----------------------------------
def _distort(model: int, K: np.ndarray, q: np.ndarray) -> np.ndarray:
    """Vectorised CameraToPixelCoordinates for observations that all use `model`.
    K: [n, size], q: [n, 3] camera-frame points.  Used to synthesise pixels."""
    if model == abi.FISHEYE:
        x, y, z = q[:, 0], q[:, 1], q[:, 2]
        r = np.sqrt(x * x + y * y)
        th = np.arctan2(r, np.abs(z))
        t2 = th * th
        thd = th * (1 + K[:, 5] * t2 + K[:, 6] * t2**2 + K[:, 7] * t2**3 + K[:, 8] * t2**4)
        s = np.where(r * r < 1e-8, 1.0, thd / np.maximum(r, 1e-300)) * np.where(z < 0, -1.0, 1.0)
        s = np.where(r * r < 1e-8, 1.0, s)
        dx, dy = s * x, s * y
        return np.stack([K[:, 0] * dx + K[:, 2] * dy + K[:, 3], K[:, 0] * K[:, 1] * dy + K[:, 4]], 1)
    nx, ny = q[:, 0] / q[:, 2], q[:, 1] / q[:, 2]
    r2 = nx * nx + ny * ny
    if model == abi.PINHOLE:
        d = 1 + r2 * (K[:, 5] + K[:, 6] * r2)
        dx, dy = nx * d, ny * d
        return np.stack([K[:, 0] * dx + K[:, 2] * dy + K[:, 3], K[:, 0] * K[:, 1] * dy + K[:, 4]], 1)
    if model == abi.PINHOLE_RADIAL_TANGENTIAL:
        rd = 1 + K[:, 5] * r2 + K[:, 6] * r2**2 + K[:, 7] * r2**3
        tx = K[:, 9] * (r2 + 2 * nx * nx) + 2 * K[:, 8] * nx * ny
        ty = K[:, 8] * (r2 + 2 * ny * ny) + 2 * K[:, 9] * nx * ny
        dx, dy = nx * rd + tx, ny * rd + ty
        return np.stack([K[:, 0] * dx + K[:, 2] * dy + K[:, 3], K[:, 0] * K[:, 1] * dy + K[:, 4]], 1)
    if model == abi.FOV:
        w = K[:, 4]
        ru = np.sqrt(r2)
        with np.errstate(divide="ignore", invalid="ignore"):
            rd = np.where(
                w < 1e-3, w * w * r2 / 3 - w * w / 12 + 1,
                np.where(r2 < 1e-3,
                         -2 * np.tan(w / 2) * (4 * r2 * np.tan(w / 2) ** 2 - 3) / (3 * w),
                         np.arctan(2 * ru * np.tan(w / 2)) / (ru * w)))
        return np.stack([K[:, 0] * rd * nx + K[:, 2], K[:, 0] * K[:, 1] * rd * ny + K[:, 3]], 1)
    # division undistortion
    ux, uy = K[:, 0] * nx, K[:, 0] * K[:, 1] * ny
    ru2 = ux * ux + uy * uy
    k = K[:, 4]
    denom = 2 * k * ru2
    inner = 1 - 4 * k * ru2
    with np.errstate(divide="ignore", invalid="ignore"):
        sc = np.where((np.abs(denom) < np.finfo(float).eps) | (inner < 0), 1.0,
                      (1 - np.sqrt(np.maximum(inner, 0))) / denom)
    return np.stack([ux * sc + K[:, 2], uy * sc + K[:, 3]], 1)


def project(problem: Problem, obs_index=None) -> np.ndarray:
    """Pixels of every observation at the problem's current parameters."""
    cam = problem.obs_camera if obs_index is None else problem.obs_camera[obs_index]
    pt = problem.obs_point if obs_index is None else problem.obs_point[obs_index]
    Rm = Rotation.from_rotvec(problem.extrinsics[:, 3:6]).as_matrix()
    X = problem.points[pt]
    a = X[:, :3] - X[:, 3:4] * problem.extrinsics[cam, :3]
    q = np.einsum("nij,nj->ni", Rm[cam], a)
    out = np.empty((cam.shape[0], 2))
    grp = problem.camera_group[cam]
    models = problem.group_model[grp]
    for m in np.unique(models):
        sel = np.nonzero(models == m)[0]
        n = abi.INTRINSICS_SIZE[m]
        K = problem.intrinsics[problem.group_offset[grp[sel]][:, None] + np.arange(n)[None, :]]
        out[sel] = _distort(int(m), K, q[sel])
    return out


# ---- visibility -------------------------------------------------------------
def _track_lengths(rng, n_cameras, n_points, n_obs, heavy_tail=0.0):
    mean_k = n_obs / n_points
    if mean_k >= n_cameras:
        return np.full(n_points, n_cameras, dtype=np.int64)
    p = 1.0 / max(mean_k - 1.0, 1.0 + 1e-9)
    k = 1 + rng.geometric(min(p, 1.0), n_points).astype(np.int64)
    k = np.clip(k, 2, n_cameras)
    if heavy_tail > 0.0:
        # a fraction `heavy_tail` of the tracks is seen by tens to hundreds of views (landmark
        # points of internet photo collections; SURVEY 8d config 4: "max k a few hundred")
        long = np.flatnonzero(rng.random(n_points) < heavy_tail)
        k[long] = np.clip(np.rint(24.0 * (1.0 + rng.pareto(1.3, long.size))), 24, min(n_cameras, 400)).astype(np.int64)
    # steer the total to exactly n_obs
    for _ in range(64):
        diff = int(n_obs - k.sum())
        if diff == 0:
            break
        if diff > 0:
            cand = np.nonzero(k < n_cameras)[0]
            pick = rng.choice(cand, size=min(diff, cand.size), replace=False)
            k[pick] += 1
        else:
            cand = np.nonzero(k > 2)[0]
            pick = rng.choice(cand, size=min(-diff, cand.size), replace=False)
            k[pick] -= 1
    if k.sum() != n_obs:
        raise ValueError("cannot realise the requested observation count")
    return k


def _visibility(rng, n_cameras, n_points, n_obs, spread, heavy_tail=0.0):
    k = _track_lengths(rng, n_cameras, n_points, n_obs, heavy_tail)
    # window width w = m*k cameras, m heavy tailed, w <= n_cameras
    m_max = np.maximum(n_cameras // k, 1)
    m = np.rint(spread * n_cameras / k * rng.lognormal(0.0, 0.9, n_points)).astype(np.int64)
    m = np.clip(m, 1, m_max)
    start = rng.integers(0, n_cameras, n_points)
    pt = np.repeat(np.arange(n_points, dtype=np.int64), k)
    first = np.cumsum(k) - k
    j = np.arange(n_obs, dtype=np.int64) - np.repeat(first, k)
    mm = np.repeat(m, k)
    off = j * mm + (rng.random(n_obs) * mm).astype(np.int64)
    cam = (np.repeat(start, k) + off) % n_cameras
    return cam.astype(np.int32), pt.astype(np.int32), k


def _visibility_street(rng, n_cameras, n_points, n_obs, spread, heavy_tail=0.0, max_window=0.14):
    """Sequence structure: the views of a track are k of the w = m k CONSECUTIVE views around the track's own place on
    the path (m >= 1, log-normal around `spread` n / k, w capped at max_window n), so two views share tracks only
    when they are neighbours on the path -- the reduced camera matrix is a band (plus the wrap-around of the closed
    path), its fill about 2 E[w] / n.  Track lengths: the geometric body of _track_lengths with a short Pareto tail
    (landmarks seen from up to ~7 % of the path), the shape of the BAL track-length histograms (mode 2, mean ~5,
    maximum a few hundred).  Returns (camera, point, k, centre view of every track, window of every track)."""
    k = _track_lengths(rng, n_cameras, n_points, n_obs, 0.0)
    if heavy_tail > 0.0:
        long = np.flatnonzero(rng.random(n_points) < heavy_tail)
        k[long] = np.clip(np.rint(16.0 * (1.0 + rng.pareto(1.6, long.size))), 16, max(int(0.07 * n_cameras), 16)).astype(np.int64)
        for _ in range(64):  # steer the total back to exactly n_obs on the short tracks
            diff = int(n_obs - k.sum())
            if diff == 0:
                break
            cand = np.flatnonzero((k < 12) if diff > 0 else ((k > 2) & (k < 12)))
            pick = rng.choice(cand, size=min(abs(diff), cand.size), replace=False)
            k[pick] += 1 if diff > 0 else -1
        if k.sum() != n_obs:
            raise ValueError("cannot realise the requested observation count")
    w_cap = max(int(max_window * n_cameras), 2)
    m = np.maximum(spread * n_cameras / k * rng.lognormal(0.0, 0.5, n_points), 1.0)
    w = np.minimum(np.maximum(np.rint(m * k).astype(np.int64), k), max(w_cap, int(k.max())))
    centre = rng.integers(0, n_cameras, n_points)
    pt = np.repeat(np.arange(n_points, dtype=np.int64), k)
    first = np.cumsum(k) - k
    j = np.arange(n_obs, dtype=np.int64) - np.repeat(first, k)
    # k distinct views out of the window: the j-th of k equal strata of the window, a random view inside the stratum
    ww, kk = np.repeat(w, k), np.repeat(k, k)
    lo = (j * ww) // kk
    hi = np.maximum(((j + 1) * ww) // kk, lo + 1)
    off = lo + (rng.random(n_obs) * (hi - lo)).astype(np.int64)
    cam = (np.repeat(centre - w // 2, k) + off) % n_cameras
    return cam.astype(np.int32), pt.astype(np.int32), k, centre, w


# ---- scenes -----------------------------------------------------------------
def _look_at(C, target, up=np.array([0.0, 1.0, 0.0])):
    z = target - C
    z /= np.linalg.norm(z, axis=1, keepdims=True)
    x = np.cross(np.broadcast_to(up, z.shape), z)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    y = np.cross(z, x)
    Rm = np.stack([x, y, z], axis=1)  # rows are the camera axes in world coordinates
    return Rotation.from_matrix(Rm).as_rotvec()


def make_problem(n_cameras: int, n_points: int, n_obs: int, seed: int, *,
                 scene: str = "ring", spread: float = 0.12, pixel_noise: float = 0.5,
                 perturb: float = 1.0, models=None, shared_group_size: int = 1, shared_group_sizes=None,
                 intrinsics_to_optimize: int = abi.INTRINSICS_DEFAULT, heavy_tail: float = 0.0) -> Problem:
    """Build a seeded synthetic problem.

    scene "allsee": the reference test recipe (config 1), every view sees every track.
    scene "ring":   landmark scene with windowed visibility (configs 2-4).
    models: optional list of (camera_model, fraction); default all PINHOLE.
    shared_group_size: >1 makes consecutive cameras share an intrinsics group.
    shared_group_sizes: (lo, hi) -- groups of consecutive cameras with sizes drawn log-uniformly from [lo, hi]
             ("intrinsics groups of 1-200 views"; a group of one view is a private group).
    perturb: scale of the initial perturbation away from the generating
             parameters (1.0 = SURVEY 8d: points/positions 0.25 % of the scene
             depth, angle-axis 0.005 rad)."""
    rng = np.random.default_rng(seed)
    if scene == "allsee":
        C = 10.0 * rng.uniform(-1, 1, (n_cameras, 3))
        aa = 0.2 * rng.uniform(-1, 1, (n_cameras, 3))
        X = rng.uniform(-1, 1, (n_points, 3))
        # keep the cloud in front of every camera: depth offset as in the
        # reference recipe, scaled with the camera spread
        X[:, 2] += 20.0 + 10.0
        cam = np.tile(np.arange(n_cameras, dtype=np.int32), n_points)
        pt = np.repeat(np.arange(n_points, dtype=np.int32), n_cameras)
        if n_obs != n_cameras * n_points:
            raise ValueError("allsee scene needs n_obs == n_cameras * n_points")
        depth = 20.0
        f = np.full(n_cameras, 800.0)
        pp = np.full((n_cameras, 2), 500.0)
        k1 = np.zeros(n_cameras)
        k2 = np.zeros(n_cameras)
    elif scene == "ring":
        radius = 100.0
        phi = (np.arange(n_cameras) + rng.uniform(-0.3, 0.3, n_cameras)) * (2 * np.pi / n_cameras)
        rr = radius * (1.0 + rng.uniform(-0.08, 0.08, n_cameras))
        C = np.stack([rr * np.cos(phi), radius * rng.uniform(-0.15, 0.15, n_cameras),
                      rr * np.sin(phi)], 1)
        target = radius * 0.1 * rng.normal(size=(n_cameras, 3))
        aa = _look_at(C, target)
        X = radius * 0.3 * rng.uniform(-1, 1, (n_points, 3))
        cam, pt, _ = _visibility(rng, n_cameras, n_points, n_obs, spread, heavy_tail)
        depth = radius
        f = rng.uniform(600, 900, n_cameras)
        pp = np.zeros((n_cameras, 2))
        k1 = rng.uniform(-0.1, 0.0, n_cameras)
        k2 = rng.uniform(0.0, 0.02, n_cameras)
    elif scene == "street":
        # A closed path (a circle whose perimeter is one unit per view) photographed from the inside out: every view
        # looks away from the centre at facades / landmarks beyond the path, a track sits in front of the middle of
        # its window of consecutive views at a depth proportional to the window (a wide window = a far landmark), so
        # every view of the window has it inside a ~100 degree field of view.  Neighbouring views share most tracks,
        # distant views none: the sequence structure of real collections -- S is a band, and the
        # chain's long-wavelength bending modes are what PCG with a block-Jacobi preconditioner is slow on.
        cam, pt, _, centre, w = _visibility_street(rng, n_cameras, n_points, n_obs, spread, heavy_tail)
        R0 = n_cameras / (2 * np.pi)
        phi = (np.arange(n_cameras) + rng.uniform(-0.2, 0.2, n_cameras)) * (2 * np.pi / n_cameras)
        rr = R0 + rng.uniform(-0.3, 0.3, n_cameras)
        C = np.stack([rr * np.cos(phi), rng.uniform(-0.3, 0.3, n_cameras), rr * np.sin(phi)], 1)
        outward = np.stack([np.cos(phi), np.zeros(n_cameras), np.sin(phi)], 1)
        aa = _look_at(C, C + 10.0 * outward + rng.normal(0.0, 0.6, (n_cameras, 3)))
        z = np.maximum(6.0, 0.55 * w) * rng.uniform(1.0, 1.6, n_points)       # depth beyond the path
        pphi = (centre + rng.uniform(-0.5, 0.5, n_points)) * (2 * np.pi / n_cameras)
        X = np.stack([(R0 + z) * np.cos(pphi), z * rng.uniform(-0.35, 0.35, n_points), (R0 + z) * np.sin(pphi)], 1)
        depth = 12.0
        f = rng.uniform(600, 900, n_cameras)
        pp = np.zeros((n_cameras, 2))
        k1 = rng.uniform(-0.1, 0.0, n_cameras)
        k2 = rng.uniform(0.0, 0.02, n_cameras)
    else:
        raise ValueError(scene)

    # intrinsics groups
    if shared_group_sizes is not None:
        lo, hi = shared_group_sizes
        grng = np.random.default_rng(seed + 7919)  # its own stream: the scene does not depend on the grouping
        camera_group = np.empty(n_cameras, dtype=np.int32)
        c = g = 0
        while c < n_cameras:
            size = int(round(np.exp(grng.uniform(np.log(lo), np.log(hi)))))
            size = max(lo, min(hi, size, n_cameras - c))
            camera_group[c:c + size] = g
            c += size
            g += 1
    elif shared_group_size > 1:
        camera_group = (np.arange(n_cameras) // shared_group_size).astype(np.int32)
    else:
        camera_group = np.arange(n_cameras, dtype=np.int32)
    n_groups = int(camera_group.max()) + 1 if n_cameras else 0
    group_model = np.zeros(n_groups, dtype=np.int32)
    if models:
        edges = np.cumsum([fr for _, fr in models])
        u = rng.random(n_groups)
        for g in range(n_groups):
            group_model[g] = models[int(np.searchsorted(edges, u[g] * edges[-1]))][0]
    sizes = np.array([abi.INTRINSICS_SIZE[m] for m in group_model], dtype=np.int32)
    group_offset = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    intr = np.zeros(int(group_offset[-1]))
    rep = np.zeros(n_groups, dtype=np.int64)  # representative camera of each group
    rep[camera_group[::-1]] = np.arange(n_cameras)[::-1]
    for g in range(n_groups):
        o, m, c = group_offset[g], group_model[g], rep[g]
        if m in (abi.PINHOLE, abi.PINHOLE_RADIAL_TANGENTIAL, abi.FISHEYE):
            intr[o:o + 5] = [f[c], 1.0, 0.0, pp[c, 0], pp[c, 1]]
            if m == abi.PINHOLE:
                intr[o + 5:o + 7] = [k1[c], k2[c]]
            elif m == abi.PINHOLE_RADIAL_TANGENTIAL:
                intr[o + 5:o + 10] = [k1[c], k2[c], 0.1 * k2[c], 1e-3 * rng.normal(), 1e-3 * rng.normal()]
            else:
                intr[o + 5:o + 9] = [0.3 * k1[c], 0.3 * k2[c], 0.0, 0.0]
        elif m == abi.FOV:
            intr[o:o + 5] = [f[c], 1.0, pp[c, 0], pp[c, 1], rng.uniform(0.05, 0.4)]
        else:
            intr[o:o + 5] = [f[c], 1.0, pp[c, 0], pp[c, 1], rng.uniform(-2e-7, 0.0)]

    points = np.concatenate([X, np.ones((n_points, 1))], 1)
    prob = Problem(
        extrinsics=np.concatenate([C, aa], 1), camera_group=camera_group,
        camera_flags=np.zeros(n_cameras, np.uint8), group_model=group_model,
        group_offset=group_offset, intrinsics=intr,
        intrinsics_constant=np.zeros(intr.shape[0], np.uint8), points=points,
        point_constant=np.zeros(n_points, np.uint8), obs_camera=cam, obs_point=pt,
        obs_xy=np.zeros((cam.shape[0], 2)))
    prob.set_intrinsics_to_optimize(intrinsics_to_optimize)

    # exact projections + pixel noise
    xy = project(prob)
    xy += pixel_noise * rng.normal(size=xy.shape)
    prob.obs_xy = np.ascontiguousarray(xy)
    prob.meta["truth"] = dict(extrinsics=prob.extrinsics.copy(), intrinsics=prob.intrinsics.copy(),
                              points=prob.points.copy())
    # initial perturbation
    s = 0.0025 * depth * perturb
    prob.points[:, :3] += s * rng.normal(size=(n_points, 3))
    prob.extrinsics[:, :3] += s * rng.normal(size=(n_cameras, 3))
    prob.extrinsics[:, 3:] += 0.005 * perturb * rng.normal(size=(n_cameras, 3))
    prob.meta.update(dict(seed=seed, scene=scene, spread=spread))
    return prob


CONFIG5_INTRINSICS = (abi.INTRINSICS_FOCAL_LENGTH | abi.INTRINSICS_PRINCIPAL_POINTS | abi.INTRINSICS_RADIAL_DISTORTION
                      | abi.INTRINSICS_TANGENTIAL_DISTORTION)


def config5(**kw) -> Problem:
    """BASELINE.json configs[4] / SURVEY 8(d) config 5: the config-4 topology (1778 views, 993 923 tracks, 5 001 946
    observations), cameras 50 % PINHOLE / 25 % PINHOLE_RADIAL_TANGENTIAL / 25 % FISHEYE, shared intrinsics groups of 2-200
    consecutive views (log-uniform sizes; "groups of 1-200 views (shared)" -- a group of one is not shared),
    intrinsics_to_optimize = ALL minus skew and aspect ratio."""
    kw.setdefault("models", [(abi.PINHOLE, 0.5), (abi.PINHOLE_RADIAL_TANGENTIAL, 0.25), (abi.FISHEYE, 0.25)])
    kw.setdefault("shared_group_sizes", (2, 200))
    kw.setdefault("intrinsics_to_optimize", CONFIG5_INTRINSICS)
    return config("venice1778", **kw)


def config(name: str, **kw) -> Problem:
    """The BASELINE.json configurations by name."""
    nc, npt, nobs = CONFIG_SIZES[name]
    if name == "tiny":
        return make_problem(nc, npt, nobs, seed=1, scene="allsee", **kw)
    seeds = {"ladybug49": 49, "alamo": 570, "venice1778": 1778, "venice1778_heavy": 1778}
    spreads = {"ladybug49": 0.35, "alamo": 0.15, "venice1778": 0.12, "venice1778_heavy": 0.12, "venice1778_street": 0.025}
    kw.setdefault("spread", spreads[name])
    if name == "venice1778_heavy":
        kw.setdefault("heavy_tail", 0.002)
    if name == "venice1778_street":
        kw.setdefault("heavy_tail", 0.002)
        return make_problem(nc, npt, nobs, seed=1778, scene="street", **kw)
    return make_problem(nc, npt, nobs, seed=seeds[name], scene="ring", **kw)


def _model_intrinsics(model, f) -> np.ndarray:
    """[n, 10] zero padded intrinsics of cameras with focal lengths f, principal point (500, 400) and a mild
    distortion in each of the five models."""
    K = np.zeros((len(model), abi.MAX_INTRINSICS))
    for p, m in enumerate(model):
        if m in (abi.PINHOLE, abi.PINHOLE_RADIAL_TANGENTIAL, abi.FISHEYE):
            K[p, :5] = [f[p], 1.0, 0.0, 500.0, 400.0]
            if m == abi.PINHOLE:
                K[p, 5:7] = [-0.05, 0.01]
            elif m == abi.PINHOLE_RADIAL_TANGENTIAL:
                K[p, 5:10] = [-0.05, 0.01, 0.001, 1e-3, -1e-3]
            else:
                K[p, 5:9] = [-0.02, 0.003, 0.0, 0.0]
        elif m == abi.FOV:
            K[p, :5] = [f[p], 1.0, 500.0, 400.0, 0.2]
        else:
            K[p, :5] = [f[p], 1.0, 500.0, 400.0, -1e-7]
    return K


def make_two_view_batch(n_pairs: int, seed: int, *, min_corr: int = 30, max_corr: int = 400,
                        models=None, free_intrinsics: float = 0.0, pixel_noise: float = 0.5,
                        point_noise: float = 0.02) -> abi.TwoViewBatch:
    """Seeded view pairs as two_view_match_geometric_verification.cc hands them to
    BundleAdjustTwoViews (:285): camera 1 at the origin looking along +z, camera 2 a baseline away
    with a small rotation, correspondences of points 4-10 units in front, pixels with noise, the
    3D points as a (noisy) triangulation.  free_intrinsics: fraction of the pairs whose focal
    lengths are optimised (TwoViewBundleAdjustmentOptions::constant_camera*_intrinsics = false)."""
    rng = np.random.default_rng(seed)
    counts = rng.integers(min_corr, max_corr + 1, n_pairs)
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    N = int(ptr[-1])
    e1 = np.zeros((n_pairs, 6))
    e2 = np.zeros((n_pairs, 6))
    e2[:, :3] = rng.normal(size=(n_pairs, 3)) * [1.0, 0.2, 0.2] + [1.0, 0, 0]
    e2[:, 3:] = 0.15 * rng.normal(size=(n_pairs, 3))
    m1 = np.zeros(n_pairs, np.int32)
    m2 = np.zeros(n_pairs, np.int32)
    if models:
        edges = np.cumsum([fr for _, fr in models])
        for arr in (m1, m2):
            u = rng.random(n_pairs) * edges[-1]
            arr[:] = [models[int(np.searchsorted(edges, x))][0] for x in u]

    def intrinsics(model):
        return _model_intrinsics(model, rng.uniform(600, 900, n_pairs))

    k1, k2 = intrinsics(m1), intrinsics(m2)
    X = np.concatenate([rng.uniform(-2, 2, (N, 2)), rng.uniform(4, 10, (N, 1)), np.ones((N, 1))], 1)
    pair_of = np.repeat(np.arange(n_pairs), counts)

    def proj(ext, model, K):
        Rm = Rotation.from_rotvec(ext[pair_of, 3:6]).as_matrix()
        a = X[:, :3] - ext[pair_of, :3]
        q = np.einsum("nij,nj->ni", Rm, a)
        out = np.empty((N, 2))
        for m in np.unique(model):
            sel = np.nonzero(model[pair_of] == m)[0]
            out[sel] = _distort(int(m), K[pair_of[sel], :abi.INTRINSICS_SIZE[m]], q[sel])
        return out

    f1 = proj(e1, m1, k1) + pixel_noise * rng.normal(size=(N, 2))
    f2 = proj(e2, m2, k2) + pixel_noise * rng.normal(size=(N, 2))
    pts = X.copy()
    pts[:, :3] += point_noise * rng.normal(size=(N, 3))
    e2_0 = e2.copy()
    e2_0[:, :3] += 0.02 * rng.normal(size=(n_pairs, 3))
    e2_0[:, 3:] += 0.004 * rng.normal(size=(n_pairs, 3))
    free = rng.random(n_pairs) < free_intrinsics
    c1 = np.where(free, 0, 1).astype(np.uint8)
    c2 = np.where(free, 0, 1).astype(np.uint8)
    k1_0, k2_0 = k1.copy(), k2.copy()
    k1_0[free, 0] *= 1.01
    k2_0[free, 0] *= 0.99
    return abi.TwoViewBatch(e1, e2_0, m1, m2, k1_0, k2_0, c1, c2, ptr, f1, f2, pts)


VERIFICATION_ROLES = ("gate1_min", "gate1_below", "gate1_tiny", "gate2", "gate2", "end_min", "end_min_plus_1",
                      "n63", "n64", "n65", "long", "long")


def make_two_view_verification_batch(n_pairs: int, seed: int, *, min_matches: int = 30, min_corr: int = 40,
                                     max_corr: int = 400, models=None, free_intrinsics: float = 0.0,
                                     pixel_noise: float = 0.5, outlier_fraction: float = 0.2, roles: bool = True,
                                     counts=None):
    """Seeded view pairs as TwoViewMatchGeometricVerification::VerifyMatches has them when it reaches
    BundleAdjustRelativePose (two_view_match_geometric_verification.cc:171-176): the two cameras of the estimated
    TwoViewInfo (camera 1 at the origin, camera 2 a baseline away, its pose a little off the truth) and the pair's
    correspondences in pixels.  The geometry is make_two_view_batch's; batch.points is zero (an output).

    Of every ordinary pair's correspondences a fraction outlier_fraction is, in equal parts, kind
      1  a gross mismatch (feature 2 anywhere in the image),
      2  a far point (60-100 units away: below the triangulation angle),
      3  a point behind both cameras,
      4  a near miss (feature 2 off by 12-24 pixels);
    kind 0 is an inlier with Gaussian pixel_noise.  roles: the first pairs (as many of VERIFICATION_ROLES as fit) are
      gate1_*         min_matches, min_matches - 1 and 3 correspondences: at or under the input gate,
      gate2           over the input gate, but most of it far points: under the gate after the triangulation,
      end_min, end_min_plus_1   exactly min_matches / min_matches + 1 clean inliers (pixel noise 0.05) among far points,
      n63, n64, n65   that many correspondences,
      long            500-900 correspondences.
    counts: the correspondences of every pair (overrides the sizes of the ordinary pairs and of n63 / n64 / n65 / long).
    Returns (batch, truth): truth["extrinsics2"] [P, 6] the generating pose, truth["kind"] [N], truth["role"] [P] (""
    for an ordinary pair), truth["points"] [N, 4]."""
    rng = np.random.default_rng(seed)
    role = [VERIFICATION_ROLES[p] if roles and p < len(VERIFICATION_ROLES) else "" for p in range(n_pairs)]
    n = rng.integers(min_corr, max_corr + 1, n_pairs)
    fixed = {"n63": 63, "n64": 64, "n65": 65}
    for p, r in enumerate(role):
        if r in fixed:
            n[p] = fixed[r]
        elif r == "long":
            n[p] = rng.integers(500, 901)
    if counts is not None:
        n = np.asarray(counts, dtype=np.int64).copy()
    kinds = []
    for p, r in enumerate(role):
        if r.startswith("gate1"):
            k = np.zeros({"gate1_min": min_matches, "gate1_below": max(min_matches - 1, 0), "gate1_tiny": 3}[r], int)
        elif r == "gate2":
            k = np.concatenate([np.zeros(max(min_matches - 5, 0), int), np.full(20, 2)])
        elif r.startswith("end_min"):
            k = np.concatenate([np.zeros(min_matches + (r == "end_min_plus_1"), int), np.full(9, 2)])
        else:
            k = np.zeros(int(n[p]), int)
            bad = rng.random(k.size) < outlier_fraction
            k[bad] = rng.integers(1, 5, int(bad.sum()))
        if r.startswith(("gate2", "end_min")):
            k = k[rng.permutation(k.size)]
        kinds.append(k)
    counts = np.array([k.size for k in kinds], dtype=np.int64)
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    kind = np.concatenate(kinds) if kinds else np.zeros(0, int)
    N = int(ptr[-1])
    e1 = np.zeros((n_pairs, 6))
    e2 = np.zeros((n_pairs, 6))
    e2[:, :3] = rng.uniform(-1, 1, (n_pairs, 3)) * [0.3, 0.15, 0.15] + [1.2, 0, 0]
    e2[:, 3:] = 0.1 * rng.normal(size=(n_pairs, 3))
    m1 = np.zeros(n_pairs, np.int32)
    m2 = np.zeros(n_pairs, np.int32)
    if models:
        edges = np.cumsum([fr for _, fr in models])
        for arr in (m1, m2):
            u = rng.random(n_pairs) * edges[-1]
            arr[:] = [models[int(np.searchsorted(edges, x))][0] for x in u]
    k1 = _model_intrinsics(m1, rng.uniform(600, 900, n_pairs))
    k2 = _model_intrinsics(m2, rng.uniform(600, 900, n_pairs))
    depth = rng.uniform(4, 8, N)
    depth[kind == 2] = rng.uniform(60, 100, int((kind == 2).sum()))
    depth[kind == 3] = -rng.uniform(4, 8, int((kind == 3).sum()))
    X = np.concatenate([rng.uniform(-0.25, 0.25, (N, 2)) * np.abs(depth)[:, None] + [[0.6, 0.0]], depth[:, None],
                        np.ones((N, 1))], 1)
    pair_of = np.repeat(np.arange(n_pairs), counts)

    def proj(ext, model, K):
        Rm = Rotation.from_rotvec(ext[pair_of, 3:6]).as_matrix()
        q = np.einsum("nij,nj->ni", Rm, X[:, :3] - ext[pair_of, :3])
        out = np.empty((N, 2))
        for m in np.unique(model):
            sel = np.nonzero(model[pair_of] == m)[0]
            out[sel] = _distort(int(m), K[pair_of[sel], :abi.INTRINSICS_SIZE[m]], q[sel])
        return out

    clean = np.array([r.startswith("end_min") for r in role], dtype=bool)
    sigma = np.where(clean[pair_of], 0.05, pixel_noise)[:, None] if N else np.zeros((0, 1))
    f1 = proj(e1, m1, k1) + sigma * rng.normal(size=(N, 2))
    f2 = proj(e2, m2, k2) + sigma * rng.normal(size=(N, 2))
    gross = kind == 1
    f2[gross] = rng.uniform([100.0, 50.0], [900.0, 750.0], (int(gross.sum()), 2))
    near = kind == 4
    phi = rng.uniform(0, 2 * np.pi, int(near.sum()))
    f2[near] += rng.uniform(12, 24, int(near.sum()))[:, None] * np.stack([np.cos(phi), np.sin(phi)], 1)
    e2_0 = e2.copy()
    e2_0[:, :3] += 0.01 * rng.normal(size=(n_pairs, 3))
    e2_0[:, 3:] += 0.002 * rng.normal(size=(n_pairs, 3))
    free = rng.random(n_pairs) < free_intrinsics
    c1 = np.where(free, 0, 1).astype(np.uint8)
    c2 = np.where(free, 0, 1).astype(np.uint8)
    k1[free, 0] *= 1.005
    k2[free, 0] *= 0.995
    batch = abi.TwoViewBatch(e1, e2_0, m1, m2, k1, k2, c1, c2, ptr, f1, f2, np.zeros((N, 4)))
    return batch, {"extrinsics2": e2, "kind": kind, "role": role, "points": X}


def make_two_view_angular_batch(n_pairs: int, seed: int, *, min_corr: int = 30, max_corr: int = 300,
                                noise: float = 1e-3, rotation_error: float = 0.03, position_error: float = 0.08,
                                rotation_scale: float = 0.05):
    """Seeded view pairs for BundleAdjustTwoViewsAngular: view 1 at the origin, view 2 at a unit-norm
    position with a small rotation, points 3-9 units in front of both; features are NORMALISED image
    coordinates (angular_epipolar_error.h works on calibrated rays) with Gaussian noise; the starting
    relative pose is the true one perturbed.  Returns (batch, true rotation [P, 3], true position [P, 3])."""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(seed)
    counts = rng.integers(min_corr, max_corr + 1, n_pairs)
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    N = int(ptr[-1])
    # small relative rotations: the functor's second term is (R f2) . T (R^T f2) as the reference writes it
    # (angular_epipolar_error.h:71-72), which only stays positive -- and the residual zero at the true pose --
    # while R f2 and R^T f2 are close
    rot_true = rotation_scale * rng.normal(size=(n_pairs, 3))
    pos_true = rng.normal(size=(n_pairs, 3)) * [1.0, 0.3, 0.3] + [1.5, 0, 0]
    pos_true /= np.linalg.norm(pos_true, axis=1, keepdims=True)
    f1 = np.zeros((N, 2))
    f2 = np.zeros((N, 2))
    for p in range(n_pairs):
        n = int(counts[p])
        X = np.stack([rng.uniform(-2.5, 2.5, n), rng.uniform(-2.0, 2.0, n), rng.uniform(3.0, 9.0, n)], 1)
        R = Rotation.from_rotvec(rot_true[p])
        X2 = R.apply(X - pos_true[p])
        f1[ptr[p]:ptr[p + 1]] = X[:, :2] / X[:, 2:3]
        f2[ptr[p]:ptr[p + 1]] = X2[:, :2] / X2[:, 2:3]
    f1 += noise * rng.normal(size=f1.shape)
    f2 += noise * rng.normal(size=f2.shape)
    rot0 = rot_true + rotation_error * rng.normal(size=rot_true.shape)
    pos0 = pos_true + position_error * rng.normal(size=pos_true.shape)
    pos0 /= np.linalg.norm(pos0, axis=1, keepdims=True)
    return abi.TwoViewAngularBatch(rot0, pos0, ptr, f1, f2), rot_true, pos_true


def make_relative_position_batch(n_pairs: int, seed: int, *, min_corr: int = 30, max_corr: int = 300,
                                 pixel_noise: float = 0.5, models=None, n_views: int = 48, counts=None):
    """Seeded view-graph edges for OptimizeRelativePositionWithKnownRotation: n_views views with known poses on the
    ring scene (radius 100, looking at the centre), every pair one to three places apart on the ring (a baseline of
    13 to 40 units against a depth of about 100) in either order, correspondences of points around the centre, in front
    of both views.  models: optional list of (camera_model, fraction) -- the views then carry a model with
    non-trivial distortion and the features are PIXELS projected through it; otherwise the features are NORMALISED
    coordinates.  pixel_noise: uniform in +-pixel_noise pixels (divided by the focal length for normalised features).
    counts: the correspondences of every pair (overrides min_corr / max_corr).
    Returns (batch, true directions R1 (C2 - C1) / |C2 - C1| [P, 3])."""
    rng = np.random.default_rng(seed)
    V = int(n_views)
    radius = 100.0
    phi = (np.arange(V) + rng.uniform(-0.3, 0.3, V)) * (2 * np.pi / V)
    rr = radius * (1.0 + rng.uniform(-0.08, 0.08, V))
    Cw = np.stack([rr * np.cos(phi), radius * rng.uniform(-0.15, 0.15, V), rr * np.sin(phi)], 1)
    aa = _look_at(Cw, radius * 0.05 * rng.normal(size=(V, 3)))
    Rm = Rotation.from_rotvec(aa).as_matrix()
    model = np.zeros(V, np.int32)
    if models:
        edges = np.cumsum([fr for _, fr in models])
        u = rng.random(V) * edges[-1]
        model[:] = [models[int(np.searchsorted(edges, x))][0] for x in u]
    f = rng.uniform(600, 900, V)
    K = _model_intrinsics(model, f)
    if counts is None:
        counts = rng.integers(min_corr, max_corr + 1, n_pairs)
    counts = np.asarray(counts, dtype=np.int64)
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    N = int(ptr[-1])
    va = rng.integers(0, V, n_pairs)
    vb = (va + rng.integers(1, 4, n_pairs)) % V
    swap = rng.random(n_pairs) < 0.5
    v1 = np.where(swap, vb, va).astype(np.int32)
    v2 = np.where(swap, va, vb).astype(np.int32)
    X = radius * 0.3 * rng.uniform(-1, 1, (N, 3))
    pair_of = np.repeat(np.arange(n_pairs), counts)

    def features(view):
        vv = view[pair_of]
        q = np.einsum("nij,nj->ni", Rm[vv], X - Cw[vv])
        noise = rng.uniform(-pixel_noise, pixel_noise, (N, 2))
        if not models:
            return q[:, :2] / q[:, 2:3] + noise / f[vv][:, None]
        out = np.empty((N, 2))
        for m in np.unique(model):
            sel = np.nonzero(model[vv] == m)[0]
            out[sel] = _distort(int(m), K[vv[sel], :abi.INTRINSICS_SIZE[m]], q[sel])
        return out + noise

    f1, f2 = features(v1), features(v2)
    d = Cw[v2] - Cw[v1]
    truth = np.einsum("nij,nj->ni", Rm[v1], d / np.linalg.norm(d, axis=1, keepdims=True))
    batch = abi.RelativePositionBatch(aa, v1, v2, ptr, f1, f2, None, model if models else None, K if models else None)
    return batch, truth


def make_view_pair_batch(num_views: int, num_valid: int, num_invalid: int, seed: int):
    """A view graph after the recipe of filter_view_pairs_from_relative_translation_test.cc:59-150 with a numpy
    generator: view 0 at the origin with identity orientation, the others with angle-axis orientation and position
    uniform in [-1, 1]^3; a skeletal path (i - 1, i), random extra valid edges (view1 < view2) up to num_valid, then
    num_invalid edges whose rotation_2 has ones added and whose position_2 is a random unit vector.  A valid edge has
    rotation_2 = AngleAxis(R2 R1^T) and position_2 = R1 (c2 - c1) / |c2 - c1| (:71-93).
    Returns (abi.ViewPairBatch, positions [V, 3]); the first num_valid edges are the valid ones."""
    rng = np.random.default_rng(seed)
    V = int(num_views)
    if num_valid < V - 1 or num_valid + num_invalid > V * (V - 1) // 2:
        raise ValueError("make_view_pair_batch: the edge counts do not fit the view count")
    aa = rng.uniform(-1.0, 1.0, (V, 3))
    pos = rng.uniform(-1.0, 1.0, (V, 3))
    aa[0] = 0.0
    pos[0] = 0.0
    Rm = Rotation.from_rotvec(aa).as_matrix()

    def info(a, b):
        d = pos[b] - pos[a]
        return Rotation.from_matrix(Rm[b] @ Rm[a].T).as_rotvec(), Rm[a] @ (d / np.linalg.norm(d))

    edges, taken, rot2, pos2 = [], set(), [], []
    for i in range(1, V):
        edges.append((i - 1, i))
        taken.add((i - 1, i))
    while len(edges) < num_valid:
        a, b = (int(x) for x in rng.choice(V, 2, replace=False))
        if a > b or (a, b) in taken:
            continue
        edges.append((a, b))
        taken.add((a, b))
    for a, b in edges:
        r, t = info(a, b)
        rot2.append(r)
        pos2.append(t)
    while len(edges) < num_valid + num_invalid:
        a, b = int(rng.integers(0, V)), int(rng.integers(0, V))
        if a >= b or (a, b) in taken:
            continue
        edges.append((a, b))
        taken.add((a, b))
        r, _ = info(a, b)
        t = rng.uniform(-1.0, 1.0, 3)
        rot2.append(r + 1.0)
        pos2.append(t / np.linalg.norm(t))
    e = np.asarray(edges, dtype=np.int32).reshape(-1, 2)
    return abi.ViewPairBatch(aa, e[:, 0], e[:, 1], np.asarray(rot2).reshape(-1, 3), np.asarray(pos2).reshape(-1, 3)), pos



def make_localization_batch(num_views: int, num_correspondences, seed: int, *, inlier_ratio=1.0, pixel_noise=0.5,
                            num_points: int = 0, models=None, threshold_pixels: float = 4.0,
                            image_size=(1000, 800)) -> Problem:
    """Candidate views to localise against a fixed point cloud (tmi_ba_localize_views): a cloud uniform in a cube of
    side 4 around the origin, V views on a sphere of radius about 8 looking at it with known poses (focal lengths
    700..900 pixels, principal point (500, 400)), view v observing num_correspondences[v] distinct points (a scalar
    serves every view).  A fraction inlier_ratio[v] of a view's observations are the projections with Gaussian noise of
    pixel_noise[v] pixels; the others are outliers, uniform over the image.  models: optional camera model per view
    (default PINHOLE without distortion).  Every view has an intrinsics group of its own, all intrinsics constant.
    The extrinsics of the returned problem are zero (the call ignores them); meta holds `true_extrinsics` [V, 6],
    `obs_is_inlier` [No] and `error_threshold` [V], the squared threshold in normalised coordinates for
    threshold_pixels on a `image_size` image (ComputeResolutionScaledThreshold / focal length, squared)."""
    rng = np.random.default_rng(seed)
    V = int(num_views)
    ncorr = np.broadcast_to(np.asarray(num_correspondences, dtype=np.int64), (V,)).copy()
    ratio = np.broadcast_to(np.asarray(inlier_ratio, dtype=np.float64), (V,))
    noise = np.broadcast_to(np.asarray(pixel_noise, dtype=np.float64), (V,))
    Np = int(num_points) if num_points else int(max(ncorr.max(initial=1), 4))
    if ncorr.max(initial=0) > Np:
        raise ValueError("make_localization_batch: a view observes more points than there are")
    X = rng.uniform(-2.0, 2.0, (Np, 3))
    d = rng.normal(size=(V, 3))
    Cpos = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(7.0, 9.0, (V, 1))
    aa = _look_at(Cpos, 0.3 * rng.normal(size=(V, 3)))
    f = rng.uniform(700.0, 900.0, V)
    model = np.zeros(V, dtype=np.int32) if models is None else np.asarray(models, dtype=np.int32)
    K = _model_intrinsics(model, f)
    if models is None:
        K[:, 5:] = 0.0
    sizes = np.asarray([abi.INTRINSICS_SIZE[m] for m in model], dtype=np.int32)
    offset = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    intr = np.concatenate([K[v, :sizes[v]] for v in range(V)]) if V else np.zeros(0)
    cam = np.repeat(np.arange(V, dtype=np.int32), ncorr)
    pt = np.concatenate([rng.permutation(Np)[:n] for n in ncorr]).astype(np.int32) if V else np.zeros(0, np.int32)
    # interleave the views' observations so that a view's are not contiguous in the caller's arrays
    order = rng.permutation(cam.shape[0])
    cam, pt = cam[order], pt[order]
    prob = Problem(np.concatenate([Cpos, aa], 1), np.arange(V, dtype=np.int32), np.zeros(V, np.uint8), model, offset,
                   intr, np.ones(intr.shape[0], np.uint8), np.concatenate([X, np.ones((Np, 1))], 1),
                   np.zeros(Np, np.uint8), cam, pt, np.zeros((cam.shape[0], 2)))
    px = project(prob) + rng.normal(size=(cam.shape[0], 2)) * noise[cam][:, None]
    is_inlier = np.ones(cam.shape[0], dtype=bool)
    for v in range(V):
        idx = np.nonzero(cam == v)[0]
        n_out = int(round((1.0 - ratio[v]) * idx.shape[0]))
        out = idx[rng.permutation(idx.shape[0])[:n_out]]
        is_inlier[out] = False
        px[out] = rng.uniform(0.0, 1.0, (n_out, 2)) * np.asarray(image_size, dtype=np.float64)
    prob.obs_xy[:] = px
    prob.meta["true_extrinsics"] = prob.extrinsics.copy()
    prob.meta["obs_is_inlier"] = is_inlier
    prob.meta["error_threshold"] = (threshold_pixels * max(image_size) / 1024.0 / f) ** 2
    prob.extrinsics[:] = 0.0
    return prob


def make_matching_batch(num_images: int, num_descriptors, dim: int, seed: int, *, match_share: float = 0.5,
                        noise: float = 0.05, num_duplicates: int = 0, num_ties: int = 0, integer: bool = False,
                        pool_size: int = 0):
    """Descriptors for tmi_ba_match_features: a pool of pool_size (0: max(num_descriptors)) unit-norm "scene"
    descriptors; image m holds num_descriptors[m] rows (a scalar serves every image), of which a share match_share are
    pool descriptors (the first ones of the pool, cyclically, so that they recur across images) with Gaussian noise of
    `noise` per element and the others are random; the rows of an image are shuffled.  integer: values are whole
    numbers 0..255 instead (every fp32 operation on them is exact for dim <= 258).
    num_duplicates: in every image with at least two rows, that many rows are overwritten with copies of other rows of
    the same image: for a query that is nearest to such a row, best == second in every bit.
    num_ties: that many rows q of image 0 are queries with two equally near columns in every other image m with at
    least two rows: rows lo and hi of image m become copies of q with element 0 moved by -e and +e (e = 1 where
    integer, else 2^-6; element 0 of q is first rounded so that both are exact), so d(q, lo) == d(q, hi) == e^2.
    Returns (image_begin int64 [num_images + 1], descriptors float32 [rows, dim], meta) with meta['duplicate_rows'] a
    list of (image, row, source row) and meta['tie_rows'] a list of (q, image, lo, hi)."""
    rng = np.random.default_rng(seed)
    n = np.broadcast_to(np.asarray(num_descriptors, dtype=np.int64), (int(num_images),)).copy()
    begin = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    pool_n = int(pool_size) if pool_size else int(n.max(initial=0))

    def draw(k):
        if integer:
            return rng.integers(0, 256, (k, dim)).astype(np.float32)
        x = rng.normal(size=(k, dim))
        return (x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12)).astype(np.float32)

    pool = draw(pool_n)
    parts, dups, ties = [], [], []
    for m in range(int(num_images)):
        k = int(n[m])
        shared = int(round(match_share * k))
        a = pool[np.arange(shared) % max(pool_n, 1)].copy() if pool_n else pool[:0].copy()
        if integer:
            a = np.clip(a + np.rint(rng.normal(size=a.shape) * noise * 255.0), 0, 255).astype(np.float32)
        else:
            a = (a + rng.normal(size=a.shape).astype(np.float32) * np.float32(noise)).astype(np.float32)
        rows = np.concatenate([a, draw(k - shared)], 0)[rng.permutation(k)] if k else np.zeros((0, dim), np.float32)
        parts.append(rows)
    used = [set() for _ in range(int(num_images))]
    e = np.float32(1.0 if integer else 2.0 ** -6)
    for q in range(min(int(num_ties), int(n[0]) if num_images else 0)):
        base = parts[0][q]
        base[0] = np.float32(min(max(base[0], 1.0), 254.0)) if integer else np.float32(np.round(base[0] * 32.0) / 32.0)
        used[0].add(q)
        for m in range(1, int(num_images)):
            free = [r for r in range(int(n[m])) if r not in used[m]]
            if len(free) < 2:
                continue
            lo, hi = (int(v) for v in rng.choice(free, 2, replace=False))
            parts[m][lo] = base
            parts[m][hi] = base
            parts[m][lo, 0] = base[0] - e
            parts[m][hi, 0] = base[0] + e
            used[m].update((lo, hi))
            ties.append((q, m, lo, hi))
    for m in range(int(num_images)):
        for _ in range(int(num_duplicates)):
            free = [r for r in range(int(n[m])) if r not in used[m]]
            if len(free) < 2:
                break
            src, dst = (int(v) for v in rng.choice(free, 2, replace=False))
            parts[m][dst] = parts[m][src]
            used[m].update((src, dst))
            dups.append((m, dst, src))
    desc = np.concatenate(parts, 0) if parts else np.zeros((0, dim), np.float32)
    return begin, np.ascontiguousarray(desc, dtype=np.float32), {"duplicate_rows": dups, "tie_rows": ties}


def _mt19937_normals(seed: int, count: int) -> np.ndarray:
    """count draws of std::normal_distribution<double>(0, 1), a FRESH distribution per draw, from std::mt19937(seed),
    as libstdc++ computes them: the Marsaglia polar method on x = 2 u - 1 with u = generate_canonical<double, 53> (two
    32-bit words, low word first), returning y * sqrt(-2 log(r2) / r2) of the pair's SECOND coordinate and dropping
    the saved one with the distribution."""
    bits = np.random.MT19937()
    state = bits.state
    key = np.zeros(624, dtype=np.uint32)
    key[0] = seed & 0xFFFFFFFF
    for i in range(1, 624):
        key[i] = (1812433253 * (int(key[i - 1]) ^ (int(key[i - 1]) >> 30)) + i) & 0xFFFFFFFF
    state["state"]["key"] = key
    state["state"]["pos"] = 624
    bits.state = state
    out = np.empty(count, dtype=np.float64)

    def canonical():
        lo = int(bits.random_raw())
        hi = int(bits.random_raw())
        r = (lo + hi * 4294967296.0) / 18446744073709551616.0
        return r if r < 1.0 else float(np.nextafter(1.0, 0.0))

    for i in range(count):
        while True:
            x = 2.0 * canonical() - 1.0
            y = 2.0 * canonical() - 1.0
            r2 = x * x + y * y
            if not (r2 > 1.0 or r2 == 0.0):
                break
        out[i] = y * np.sqrt(-2.0 * np.log(r2) / r2)
    return out


CASCADE_DEFAULT_SEED = 20140623  # theia::CascadeHashingFeatureMatcher's default seed


def cascade_projections(dim: int, seed: int = CASCADE_DEFAULT_SEED, *, zero_secondary: bool = False) -> np.ndarray:
    """The projections of tmi_ba_match_features_cascade, [188, dim] float32, as theia::CascadeHashingFeatureMatcher
    draws them from `seed`: std::mt19937(seed), a fresh std::normal_distribution<double>(0, 1) per draw cast to float,
    the primary projection's 128 rows first, then bit k of group g at row 128 + 10 g + k, each row in ascending
    dimension (CascadeHasher::Initialize).  zero_secondary: rows 128.. are all zero, so that every row of every image
    falls into bucket 0 of every group (a test input)."""
    p = _mt19937_normals(int(seed), 188 * int(dim)).astype(np.float32).reshape(188, int(dim))
    if zero_secondary:
        p[128:] = 0.0
    return np.ascontiguousarray(p)


def make_uncalibrated_pair_batch(num_pairs: int, num_correspondences, seed: int, *, inlier_ratio=1.0, pixel_noise=0.5,
                                 focal_range=(800.0, 1600.0), image_half_size=(512.0, 384.0), parallel_axes=()):
    """View pairs for tmi_ba_estimate_uncalibrated_relative_poses: two pinhole views with DIFFERENT focal lengths drawn
    from focal_range and NON-PARALLEL optical axes that do not meet (view 2 is turned about x and y and moved along all
    three axes; otherwise the focal lengths are not recoverable from F), scene points in front of both views and inside
    both images, CENTRED pixels (principal point (0, 0)) with Gaussian pixel_noise, and outliers (a share
    1 - inlier_ratio of every pair, exactly round(...) of them) uniform in the two images.  num_correspondences and
    inlier_ratio: a scalar or one value per pair.  parallel_axes: pair indices whose view 2 is NOT turned (the degenerate configuration).
    Returns a dict: pair_offset [P + 1] int64, feature1 / feature2 [N, 2], is_inlier [N] bool, focal_length1 /
    focal_length2 [P], rotation [P, 3] (angle-axis of view 2), position [P, 3] (unit norm), fundamental_matrix
    [P, 3, 3] (x2^T F x1 = 0, unit Frobenius norm), points [N, 3] (in view 1's frame)."""
    rng = np.random.default_rng(seed)
    n = np.broadcast_to(np.asarray(num_correspondences, dtype=np.int64), (int(num_pairs),)).copy()
    ratio = np.broadcast_to(np.asarray(inlier_ratio, dtype=np.float64), (int(num_pairs),))
    ptr = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    N = int(ptr[-1])
    f1 = np.zeros((N, 2))
    f2 = np.zeros((N, 2))
    X = np.zeros((N, 3))
    inl = np.zeros(N, dtype=bool)
    fl1 = rng.uniform(focal_range[0], focal_range[1], num_pairs)
    fl2 = rng.uniform(focal_range[0], focal_range[1], num_pairs)
    rot = np.zeros((num_pairs, 3))
    pos = np.zeros((num_pairs, 3))
    Fm = np.zeros((num_pairs, 3, 3))
    hw, hh = image_half_size
    for p in range(int(num_pairs)):
        sign = rng.choice([-1.0, 1.0], 2)
        aa = np.array([sign[0] * rng.uniform(0.08, 0.2), -rng.uniform(0.15, 0.35), rng.uniform(-0.1, 0.1)])
        if p in parallel_axes:
            aa[:] = 0.0
        c = np.array([rng.uniform(0.8, 1.4), sign[1] * rng.uniform(0.3, 0.6), rng.uniform(-0.3, 0.3)])
        R = Rotation.from_rotvec(aa).as_matrix()
        rot[p] = aa
        pos[p] = c / np.linalg.norm(c)
        tx = np.array([[0, -c[2], c[1]], [c[2], 0, -c[0]], [-c[1], c[0], 0]])
        E = R @ tx.T  # x2^T E x1 = 0 for x2 ~ R (X - c): E = [t]_x R with t = -R c, i.e. R [c]_x^T
        Fp = np.diag([1 / fl2[p], 1 / fl2[p], 1.0]) @ E @ np.diag([1 / fl1[p], 1 / fl1[p], 1.0])
        Fm[p] = Fp / np.linalg.norm(Fp)
        k = int(n[p])
        got = 0
        a, b = int(ptr[p]), int(ptr[p + 1])
        while got < k:
            m = 4 * (k - got) + 16
            depth = rng.uniform(4.0, 9.0, m)
            Y = np.stack([rng.uniform(-hw, hw, m) / fl1[p] * depth, rng.uniform(-hh, hh, m) / fl1[p] * depth, depth], 1)
            q = (Y - c) @ R.T
            u2 = fl2[p] * q[:, :2] / q[:, 2:3]
            ok = (q[:, 2] > 1.0) & (np.abs(u2[:, 0]) < hw) & (np.abs(u2[:, 1]) < hh)
            take = np.nonzero(ok)[0][:k - got]
            X[a + got:a + got + take.size] = Y[take]
            f1[a + got:a + got + take.size] = fl1[p] * Y[take, :2] / Y[take, 2:3]
            f2[a + got:a + got + take.size] = u2[take]
            got += take.size
        f1[a:b] += pixel_noise * rng.normal(size=(k, 2))
        f2[a:b] += pixel_noise * rng.normal(size=(k, 2))
        n_out = int(round((1.0 - float(ratio[p])) * k))
        out = rng.permutation(k)[:n_out]
        inl[a:b] = True
        inl[a + out] = False
        f1[a + out] = rng.uniform([-hw, -hh], [hw, hh], (n_out, 2))
        f2[a + out] = rng.uniform([-hw, -hh], [hw, hh], (n_out, 2))
    return dict(pair_offset=ptr, feature1=f1, feature2=f2, is_inlier=inl, focal_length1=fl1, focal_length2=fl2,
                rotation=rot, position=pos, fundamental_matrix=Fm, points=X)


def make_calibrated_pair_batch(num_pairs: int, num_correspondences, seed: int, *, inlier_ratio=1.0, pixel_noise=0.5,
                               focal_range=(800.0, 1600.0), image_half_size=(512.0, 384.0)):
    """View pairs for tmi_ba_estimate_calibrated_relative_poses: the scenes of make_uncalibrated_pair_batch (same
    arguments, same random stream) with every feature divided by its view's focal length, i.e. NORMALISED coordinates
    with pixel_noise / focal of noise.  Returns that dict with feature1 / feature2 normalised, plus pixel1 / pixel2 (the
    centred pixels) and essential_matrix [P, 3, 3] (x2^T E x1 = 0, unit Frobenius norm)."""
    b = make_uncalibrated_pair_batch(num_pairs, num_correspondences, seed, inlier_ratio=inlier_ratio,
                                     pixel_noise=pixel_noise, focal_range=focal_range, image_half_size=image_half_size)
    ptr = b["pair_offset"]
    n = np.diff(ptr)
    b["pixel1"], b["pixel2"] = b["feature1"], b["feature2"]
    b["feature1"] = b["pixel1"] / np.repeat(b["focal_length1"], n)[:, None]
    b["feature2"] = b["pixel2"] / np.repeat(b["focal_length2"], n)[:, None]
    E = np.zeros((int(num_pairs), 3, 3))
    for p in range(int(num_pairs)):
        R = Rotation.from_rotvec(b["rotation"][p]).as_matrix()
        c = b["position"][p]
        tx = np.array([[0, -c[2], c[1]], [c[2], 0, -c[0]], [-c[1], c[0], 0]])
        Ep = R @ tx.T
        E[p] = Ep / np.linalg.norm(Ep)
    b["essential_matrix"] = E
    return b
