"""-m gpu: the batched TrackEstimator (tmi_ba_estimate_tracks / tmi_ba_solver_estimate_tracks) against its CPU
restatement (tests/track_estimator_model.py: oracle.pixel_to_camera, the midpoint with Eigen's LLT rule,
oracle.adjust_tracks, oracle.project_point).

Statuses must be equal; points 1e-9 relative (to max(|X|, 1)); points of tracks with status -1, 1 or 2 must be
the input bits.  Also: the resident form equals the one-shot form, a BA -> filter -> estimate -> BA chain on one
handle equals the same chain on the oracle, and tmi_ba_adjust_tracks still gives the bits recorded before the
track BA kernel took its skip mask (tests/golden/adjust_tracks_skipmask.npz)."""
import math
import os

import numpy as np
import pytest

import track_estimator_model as model
from oracle import oracle
from theiasfm_amd import abi, lib, synth

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adjust_tracks_skipmask.npz")
MIXED = [(abi.PINHOLE, 0.4), (abi.PINHOLE_RADIAL_TANGENTIAL, 0.15), (abi.FISHEYE, 0.15),
         (abi.FOV, 0.15), (abi.DIVISION_UNDISTORTION, 0.15)]


def ba_options(point_dof=4, loss=abi.LOSS_TRIVIAL, **kw):
    kw.setdefault("linear_solver_type", abi.DENSE_QR)
    kw.setdefault("use_inner_iterations", 0)
    return abi.default_options(point_dof=point_dof, loss_function_type=loss, **kw)


def scene(seed, models=None, share=1, n_cam=16, n_pts=800, n_obs=3800):
    """Ring scene with every status present: gross feature errors (bad reprojection), far-away points seen
    consistently (insufficient angle), short tracks."""
    P = synth.make_problem(n_cam, n_pts, n_obs, seed=seed, scene="ring", spread=0.3, models=models,
                           shared_group_size=share, perturb=0.2)
    rng = np.random.default_rng(seed + 200)
    n = P.num_points
    far = rng.random(n) < 0.05
    P.points[far, :3] *= 400.0
    for o in np.flatnonzero(far[P.obs_point]):
        cam = int(P.obs_camera[o])
        mdl, K = model.camera_intrinsics(P, cam)
        px, _ = oracle.project_point(mdl, P.extrinsics[cam], K, P.points[P.obs_point[o]])
        if np.all(np.isfinite(px)):
            P.obs_xy[o] = px
    bad = rng.random(P.num_observations) < 0.03
    P.obs_xy[bad] += rng.normal(0, 30.0, (int(bad.sum()), 2))
    return P


def scramble(P, mask, seed):
    """the input point of a selected track is ignored: overwrite it"""
    rng = np.random.default_rng(seed)
    sel = np.ones(P.num_points, bool) if mask is None else mask.astype(bool)
    P.points[sel] = rng.normal(0, 50.0, (int(sel.sum()), 4))


def rel_err(a, b, sel):
    if not sel.any():
        return 0.0
    scale = np.maximum(np.linalg.norm(b[sel], axis=1), 1.0)[:, None]
    return float(np.nanmax(np.abs(a[sel] - b[sel]) / scale))


def check(P, eo, bo, mask=None):
    """device one-shot vs the model on P; returns (status, points) of the device.

    Triangulated points agree with the model to 1e-9.  A point the track BA moved is compared twice: with the
    device's own tmi_ba_adjust_tracks started from the device's triangulation (the same kernel: 1e-12), and with
    oracle.adjust_tracks through the model -- there two fp64 trust-region runs on a 2-3 view track with a narrow
    valley along the viewing direction stop at slightly different places (the bar is 1e-5)."""
    ref_status, ref_points = model.estimate(P, eo, bo, mask)
    dev = P.copy()
    status, es = lib.estimate_tracks(dev, eo, bo, mask)
    np.testing.assert_array_equal(status, ref_status)
    written = np.isin(status, (0, 3, 4))
    np.testing.assert_array_equal(dev.points[~written], P.points[~written])
    if eo.bundle_adjustment:
        tri = P.copy()
        tri_status, _ = lib.estimate_tracks(tri, abi.track_estimator_options(
            max_acceptable_reprojection_error_pixels=eo.max_acceptable_reprojection_error_pixels,
            min_triangulation_angle_degrees=eo.min_triangulation_angle_degrees, bundle_adjustment=0), bo, mask)
        adjusted = np.isin(tri_status, (0, 4))  # triangulated: the tracks the track BA runs on
        assert np.array_equal(status == 3, adjusted & (status == 3))
        tri.point_constant[:] = (~adjusted).astype(np.uint8)
        term, _, _, _, _ = lib.adjust_tracks(tri, bo)
        np.testing.assert_array_equal(status[adjusted] == 3, (term[adjusted] != 0) & (term[adjusted] != 1))
        assert rel_err(dev.points, tri.points, adjusted) <= 1e-12
        moved = adjusted & (status != 3)
        assert rel_err(dev.points, ref_points, written & ~moved) <= 1e-9
        assert rel_err(dev.points, ref_points, moved) <= 1e-5
    else:
        assert rel_err(dev.points, ref_points, written) <= 1e-9
    counts = [int((status == c).sum()) for c in range(5)]
    assert es.num_attempts == int((status >= 0).sum())
    assert [es.num_estimated, es.num_bad_angle, es.num_failed_triangulation, es.num_failed_ba,
            es.num_bad_reprojection] == counts
    return status, dev.points


CASES = [(models, share, ba, dof, loss, masked)
         for models, share in ((None, 1), (MIXED, 1), (None, 4), (MIXED, 3))
         for ba in (1, 0)
         for dof, loss in ((4, abi.LOSS_TRIVIAL), (3, abi.LOSS_HUBER))
         for masked in (False, True)]


@pytest.mark.parametrize("models,share,ba,dof,loss,masked", CASES,
                         ids=[f"{'mixed' if m else 'pinhole'}-g{s}-ba{b}-dof{d}-loss{l}-{'mask' if k else 'all'}"
                              for m, s, b, d, l, k in CASES])
def test_matches_model(models, share, ba, dof, loss, masked):
    seed = 11 + 7 * share + (3 if models else 0)
    P = scene(seed, models=models, share=share)
    mask = None
    if masked:
        mask = (np.random.default_rng(seed).random(P.num_points) < 0.4).astype(np.uint8)
    scramble(P, mask, seed + 1)
    eo = abi.track_estimator_options(bundle_adjustment=ba)
    status, _ = check(P, eo, ba_options(dof, loss), mask)
    if masked:
        assert np.all(status[mask == 0] == -1)
    assert (status >= 0).sum() == (int(mask.sum()) if masked else P.num_points)
    assert (status == 0).sum() > 0.3 * (status >= 0).sum()
    if not masked:
        assert (status == 1).any() and (status == 4).any()


def test_constant_points_are_not_attempted():
    P = scene(5)
    P.point_constant[::3] = 1
    status, _ = check(P, abi.track_estimator_options(), ba_options())
    assert np.all(status[::3] == -1)


def test_iteration_limit_is_success():
    """NO_CONVERGENCE of the track BA (max_num_iterations = 1) is a usable result: acceptance still runs"""
    P = scene(6, models=MIXED)
    scramble(P, None, 3)
    status, _ = check(P, abi.track_estimator_options(), ba_options(max_num_iterations=1))
    assert (status == 0).any()


# ---- built edge cases -----------------------------------------------------------------------------------------
F, PP = 500.0, 250.0


def edge_problem(cams, tracks, K=(F, 1.0, 0.0, PP, PP, 0.0, 0.0)):
    """cams: [(position, angle-axis)]; tracks: [[(cam, (u, v))]], PINHOLE, private intrinsics."""
    nc = len(cams)
    ext = np.array([list(c) + list(a) for c, a in cams], dtype=np.float64)
    obs_c, obs_p, xy = [], [], []
    for t, tr in enumerate(tracks):
        for c, px in tr:
            obs_c.append(c)
            obs_p.append(t)
            xy.append(px)
    nk = len(K)
    return abi.Problem(ext, np.arange(nc, dtype=np.int32), np.zeros(nc, np.uint8), np.zeros(nc, np.int32),
                       np.arange(nc + 1, dtype=np.int32) * nk, np.tile(np.asarray(K, np.float64), nc),
                       np.ones(nc * nk, np.uint8), np.zeros((len(tracks), 4)) + [0, 0, 0, 1],
                       np.zeros(len(tracks), np.uint8), np.asarray(obs_c, np.int32), np.asarray(obs_p, np.int32),
                       np.asarray(xy, np.float64).reshape(-1, 2))


def proj(P, cam, X):
    mdl, K = model.camera_intrinsics(P, cam)
    px, _ = oracle.project_point(mdl, P.extrinsics[cam], K, np.asarray(X, np.float64))
    return tuple(px)


def edge_cases():
    a_hi = 20.0 * math.tan(math.radians(3.02 / 2))  # 3.02 degrees between the two rays
    a_lo = 20.0 * math.tan(math.radians(2.98 / 2))
    cams = [((0, 0, 0), (0, 0, 0)), ((1, 0, 0), (0, 0, 0)),
            ((-a_hi, 0, 0), (0, 0, 0)), ((a_hi, 0, 0), (0, 0, 0)),
            ((-a_lo, 0, 0), (0, 0, 0)), ((a_lo, 0, 0), (0, 0, 0)),
            ((-1, 0, 0), (0, 0, 0)), ((1, 0, 0), (0, 0.0, 1e-9)),
            ((0, 0, -10), (0.01, -0.02, 0.0)), ((3, 0, -10), (0.0, 0.05, 0.01))]
    P = edge_problem(cams, [[]])
    X = (0.0, 0.0, 20.0)
    tracks = [
        [],                                                   # 0: no observation -> 1
        [(1, (260.0, 240.0))],                                # 1: one observation -> 1
        [(0, (PP, PP)), (1, (PP, PP))],                       # 2: parallel rays -> 1
        [(2, proj(P, 2, X + (1.0,))), (3, proj(P, 3, X + (1.0,)))],  # 3: 3.02 degrees -> estimated
        [(4, proj(P, 4, X + (1.0,))), (5, proj(P, 5, X + (1.0,)))],  # 4: 2.98 degrees -> 1
        [(6, (PP - 0.2 * F, PP)), (7, (PP + 0.2 * F, PP))],   # 5: diverging rays, midpoint behind -> 4
        # 6: the rays of views 8 and 9 meet at the centre of view 0: the residual of view 0 cannot be
        # evaluated at the triangulated point (track BA fails at its start point -> 3)
        [(0, (300.0, 200.0)), (8, proj(P, 8, (0, 0, 0, 1))), (9, proj(P, 9, (0, 0, 0, 1)))],
    ]
    return edge_problem(cams, tracks)


@pytest.mark.parametrize("ba", [1, 0])
def test_edge_cases(ba):
    P = edge_cases()
    status, points = check(P, abi.track_estimator_options(bundle_adjustment=ba), ba_options())
    assert list(status[:6]) == [1, 1, 1, 0, 1, 4]
    assert status[6] == (3 if ba else 4)
    np.testing.assert_allclose(points[5, :3] / points[5, 3], [0, 0, -5], atol=1e-8)


def test_long_tracks():
    """every track seen by 80 views: the 16- and 64-lanes-per-track slices"""
    P = synth.make_problem(80, 300, 24000, seed=21, scene="allsee", perturb=0.2)
    scramble(P, None, 4)
    for ba in (1, 0):
        status, _ = check(P, abi.track_estimator_options(bundle_adjustment=ba), ba_options())
        assert (status == 0).all()


def test_slow_undistortion():
    """PINHOLE k1 = -0.25 at normalised radii up to 1.15: the fixed-point undistortion takes tens of steps and
    at the widest angles stops at its 100-step limit without meeting the 1e-10 test"""
    rng = np.random.default_rng(9)
    cams = [((x, 0.0, 0.0), (0.0, 0.02 * x, 0.0)) for x in (-1.0, -0.3, 0.4, 1.0)]
    K = (F, 1.0, 0.0, PP, PP, -0.25, 0.0)
    P = edge_problem(cams, [[]], K)
    tracks = []
    for _ in range(60):
        r = rng.uniform(0.2, 1.15)
        phi = rng.uniform(0, 2 * np.pi)
        z = rng.uniform(5, 15)
        X = (r * z * math.cos(phi), r * z * math.sin(phi), z, 1.0)
        tracks.append([(c, proj(P, c, X)) for c in range(4)])
    P = edge_problem(cams, tracks, K)
    for ba in (1, 0):
        check(P, abi.track_estimator_options(bundle_adjustment=ba, min_triangulation_angle_degrees=1.0),
              ba_options())


# ---- resident form --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dof", [4, 3])
def test_resident_equals_one_shot(dof):
    P = scene(31, models=MIXED, share=2)
    mask = (np.random.default_rng(1).random(P.num_points) < 0.5).astype(np.uint8)
    scramble(P, mask, 2)
    eo = abi.track_estimator_options()
    bo = ba_options(dof)
    one = P.copy()
    st1, es1 = lib.estimate_tracks(one, eo, bo, mask)
    res = P.copy()
    s = lib.Solver(res, abi.default_options(point_dof=dof, linear_solver_type=abi.ITERATIVE_SCHUR, device=0))
    try:
        st2, es2 = s.estimate_tracks(eo, bo, mask)
        s.download()
    finally:
        s.close()
    np.testing.assert_array_equal(st1, st2)
    np.testing.assert_allclose(res.points, one.points, rtol=1e-12, atol=1e-12)
    assert es1.num_estimated == es2.num_estimated and es1.num_attempts == es2.num_attempts


def test_resident_argument_errors():
    P = scene(3)
    s = lib.Solver(P, abi.default_options(point_dof=4, device=0))
    try:
        with pytest.raises(lib.EngineError) as e:
            s.estimate_tracks(abi.track_estimator_options(), ba_options(3))
        assert e.value.status == abi.ERR_INVALID_ARGUMENT
    finally:
        s.close()


def test_chain_ba_filter_estimate_ba():
    """solve -> SetOutlierTracksToUnestimated -> estimate the flagged tracks -> solve, on one resident handle and
    on the oracle + model"""
    P = synth.make_problem(12, 600, 3000, seed=7, scene="ring", spread=0.4)
    rng = np.random.default_rng(8)
    bad = rng.random(P.num_observations) < 0.02
    P.obs_xy[bad] += rng.normal(0, 20.0, (int(bad.sum()), 2))
    opts = abi.default_options(point_dof=3, linear_solver_type=abi.ITERATIVE_SCHUR, device=0)
    eo = abi.track_estimator_options(max_acceptable_reprojection_error_pixels=4.0)
    bo = ba_options(3)
    # device
    dev = P.copy()
    s = lib.Solver(dev, opts)
    try:
        st, s1 = s.solve(opts)
        assert st == 0 and s1.success
        flag, _, _ = s.filter_outlier_tracks(4.0, 2.0)
        mask = (flag != 0).astype(np.uint8)
        assert mask.any()
        status_d, _ = s.estimate_tracks(eo, bo, mask)
        st, s2 = s.solve(opts)
        assert st == 0 and s2.success
        s.download()
    finally:
        s.close()
    # oracle
    ref = P.copy()
    st, o1 = oracle.solve(ref, opts)
    assert st == 0
    flag_o, _, _ = oracle.filter_outlier_tracks(ref, 4.0, 2.0)
    np.testing.assert_array_equal(flag, flag_o)
    status_o, pts = model.estimate(ref, eo, bo, (flag_o != 0).astype(np.uint8))
    np.testing.assert_array_equal(status_d, status_o)
    ref.points[:] = pts
    st, o2 = oracle.solve(ref, opts)
    assert st == 0
    assert abs(s2.final_cost - o2.final_cost) <= 1e-6 * o2.final_cost
    scale = np.maximum(np.linalg.norm(ref.points, axis=1), 1.0)[:, None]
    assert np.max(np.abs(dev.points - ref.points) / scale) <= 1e-6


# ---- tmi_ba_adjust_tracks is unchanged by the skip mask ---------------------------------------------------------
def adjust_tracks_cases():
    """(name, problem, options) of the bit-identity check; tests/golden/adjust_tracks_skipmask.npz holds what
    tmi_ba_adjust_tracks returned for them before track_lm_kernel took its skip mask"""
    out = []
    for name, models, dof, loss in (("pinhole_dof3", None, 3, abi.LOSS_TRIVIAL),
                                    ("pinhole_dof4_huber", None, 4, abi.LOSS_HUBER),
                                    ("mixed_dof4", MIXED, 4, abi.LOSS_TRIVIAL),
                                    ("mixed_dof3_huber", MIXED, 3, abi.LOSS_HUBER)):
        P = scene(41, models=models, n_pts=800, n_obs=4000)
        P.point_constant[::7] = 1
        out.append((name, P, ba_options(dof, loss)))
    return out


def test_adjust_tracks_bits_unchanged():
    g = np.load(GOLDEN)
    for name, P, o in adjust_tracks_cases():
        term, iters, c0, c1, _ = lib.adjust_tracks(P, o)
        for key, val in (("term", term), ("iters", iters), ("c0", c0), ("c1", c1), ("points", P.points)):
            ref = g[name + "/" + key]
            assert val.dtype == ref.dtype and val.shape == ref.shape, (name, key)
            assert val.tobytes() == ref.tobytes(), (name, key)
