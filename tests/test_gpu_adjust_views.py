"""-m gpu: the batched BundleAdjustView (tmi_ba_adjust_views / tmi_ba_solver_adjust_views) against the per-view
path it replaces: every selected view's one-view subproblem (the view, its observations, their points held
constant, its intrinsics group) solved in ascending index order, each from the parameters the previous ones left,
by the device's own tmi_ba_solve and by the CPU oracle (DENSE_QR, no inner iterations, the same options).

Tolerances as in test_gpu_tracks.py: termination codes and iteration counts equal, costs 1e-9 relative,
parameters 1e-8 relative to the scene scale."""
import numpy as np
import pytest

from oracle import oracle
from theiasfm_amd import abi, lib, synth

pytestmark = pytest.mark.gpu

MODELS = [(abi.PINHOLE, 0.4), (abi.PINHOLE_RADIAL_TANGENTIAL, 0.15), (abi.FISHEYE, 0.15),
          (abi.FOV, 0.15), (abi.DIVISION_UNDISTORTION, 0.15)]
EVALUATION_FAILED = 6


def options(**kw):
    kw.setdefault("linear_solver_type", abi.DENSE_QR)
    kw.setdefault("use_inner_iterations", 0)
    return abi.default_options(**kw)


def scene(seed, n_cam=12, n_pts=1500, n_obs=8000, models=None, share=1, mask=abi.INTRINSICS_DEFAULT):
    P = synth.make_problem(n_cam, n_pts, n_obs, seed=seed, scene="ring", spread=0.3, models=models,
                           shared_group_size=share, intrinsics_to_optimize=mask, perturb=1.0)
    P.point_constant[:] = 0  # the batch holds every point constant whatever the flags say
    return P


def subproblem(P, c):
    """The one-view problem BundleAdjustView builds for view c (bundle_adjuster.cc:102-135)."""
    g = int(P.camera_group[c])
    a, b = int(P.group_offset[g]), int(P.group_offset[g + 1])
    obs = np.flatnonzero(P.obs_camera == c)
    pts, inv = np.unique(P.obs_point[obs], return_inverse=True)
    sub = abi.Problem(P.extrinsics[c:c + 1].copy(), np.zeros(1, np.int32), P.camera_flags[c:c + 1].copy(),
                      P.group_model[g:g + 1].copy(), np.array([0, b - a], np.int32), P.intrinsics[a:b].copy(),
                      P.intrinsics_constant[a:b].copy(), P.points[pts].copy(), np.ones(len(pts), np.uint8),
                      np.zeros(len(obs), np.int32), inv.astype(np.int32), P.obs_xy[obs].copy())
    return sub, a, b


def free_count(P, c):
    g = int(P.camera_group[c])
    f = int(P.camera_flags[c])
    n = (0 if f & abi.CAMERA_POSITION_CONSTANT else 3) + (0 if f & abi.CAMERA_ORIENTATION_CONSTANT else 3)
    return n + int((P.intrinsics_constant[P.group_offset[g]:P.group_offset[g + 1]] == 0).sum())


def sequential(P, opts, view_mask=None, solver=lib.solve):
    """The per-view path in ascending index order; P is updated in place.  Returns (term, iters, c0, c1)."""
    n = P.num_cameras
    term = np.full(n, -1, np.int8)
    iters = np.zeros(n, np.int32)
    c0 = np.zeros(n)
    c1 = np.zeros(n)
    for c in range(n):
        if view_mask is not None and not view_mask[c]:
            continue
        if free_count(P, c) == 0 or not np.any(P.obs_camera == c):
            continue
        sub, a, b = subproblem(P, c)
        st, s = solver(sub, opts)
        if st == EVALUATION_FAILED:
            term[c] = 3
            continue
        term[c] = s.termination
        iters[c] = s.num_iterations
        c0[c] = s.initial_cost
        c1[c] = s.final_cost
        if s.success:
            P.extrinsics[c] = sub.extrinsics[0]
            P.intrinsics[a:b] = sub.intrinsics
    return term, iters, c0, c1


def check(dev, ref, Pd, Pr, what=""):
    term_d, it_d, c0_d, c1_d = dev[:4]
    term_r, it_r, c0_r, c1_r = ref
    np.testing.assert_array_equal(term_d, term_r, err_msg=what)
    np.testing.assert_array_equal(it_d, it_r, err_msg=what)
    np.testing.assert_allclose(c0_d, c0_r, rtol=1e-9, atol=0, err_msg=what)
    np.testing.assert_allclose(c1_d, c1_r, rtol=1e-9, atol=0, err_msg=what)
    scale = float(np.abs(Pr.extrinsics[:, :3]).max())
    np.testing.assert_allclose(Pd.extrinsics, Pr.extrinsics, rtol=0, atol=1e-8 * scale, err_msg=what)
    # intrinsics: every entry relative to its own magnitude (focal lengths and distortion coefficients alike)
    np.testing.assert_allclose(Pd.intrinsics, Pr.intrinsics, rtol=1e-8, atol=1e-10, err_msg=what)


def run_all(P, opts, view_mask=None):
    """batched call vs device per-view path vs oracle per-view path, on three copies of P"""
    Pd, Pl, Po = P.copy(), P.copy(), P.copy()
    dev = lib.adjust_views(Pd, opts, view_mask)
    ref = sequential(Pl, opts, view_mask)
    check(dev, ref, Pd, Pl, "batched vs per-view device path")
    ora = sequential(Po, opts, view_mask, solver=oracle.solve)
    check(dev, ora, Pd, Po, "batched vs per-view oracle")
    return dev, Pd


@pytest.mark.parametrize("mask", [abi.INTRINSICS_DEFAULT, abi.INTRINSICS_NONE])
def test_five_models(mask):
    dev, _ = run_all(scene(1, models=MODELS, mask=mask), options())
    assert (dev[0] >= 0).all() and dev[4].num_views == 12


def test_all_intrinsics_free_d16():
    P = scene(2, models=[(abi.PINHOLE_RADIAL_TANGENTIAL, 1.0)], mask=abi.INTRINSICS_ALL)
    dev, _ = run_all(P, options())
    assert (dev[0] >= 0).all()


@pytest.mark.parametrize("loss", [abi.LOSS_TRIVIAL, abi.LOSS_HUBER, abi.LOSS_SOFTLONE, abi.LOSS_CAUCHY,
                                  abi.LOSS_ARCTAN, abi.LOSS_TUKEY])
def test_losses(loss):
    P = scene(3, models=MODELS)
    rng = np.random.default_rng(3)
    bad = rng.random(P.num_observations) < 0.05
    P.obs_xy[bad] += rng.normal(0, 20.0, (int(bad.sum()), 2))
    run_all(P, options(loss_function_type=loss, robust_loss_width=4.0))


def test_camera_flags():
    P = scene(4, models=MODELS)
    P.camera_flags[0::3] = abi.CAMERA_ORIENTATION_CONSTANT
    P.camera_flags[1::3] = abi.CAMERA_POSITION_CONSTANT
    ext0 = P.extrinsics.copy()
    _, Pd = run_all(P, options())
    assert np.array_equal(Pd.extrinsics[0::3, 3:], ext0[0::3, 3:])
    assert np.array_equal(Pd.extrinsics[1::3, :3], ext0[1::3, :3])


def test_view_mask_subset():
    P = scene(5, models=MODELS)
    mask = np.zeros(P.num_cameras, np.uint8)
    mask[[1, 4, 5, 9]] = 1
    dev, Pd = run_all(P, options(), view_mask=mask)
    assert (dev[0][mask == 0] == -1).all() and (dev[0][mask == 1] >= 0).all()
    assert np.array_equal(Pd.extrinsics[mask == 0], P.extrinsics[mask == 0])
    assert np.array_equal(Pd.points, P.points)


@pytest.mark.parametrize("share", [3, 8])
def test_shared_group_chains(share):
    """Views of a group with free entries run in sequence: the later ones start from updated intrinsics."""
    P = scene(6, n_cam=2 * share, models=[(abi.PINHOLE, 1.0)], share=share)
    assert P.num_groups == 2
    P.intrinsics[P.group_offset[:-1]] *= 1.03  # focal lengths off: the first view of a chain moves them
    dev, Pd = run_all(P, options())
    assert dev[4].num_chains == 2
    assert not np.array_equal(Pd.intrinsics, P.intrinsics)
    # a kernel that started every view from the original intrinsics (concurrent views) starts the later views
    # of a chain from other costs
    c0 = np.array([lib.solve(subproblem(P, c)[0], options())[1].initial_cost for c in range(P.num_cameras)])
    later = np.arange(P.num_cameras) % share != 0
    np.testing.assert_allclose(c0[~later], dev[2][~later], rtol=1e-9)
    assert np.all(np.abs(c0[later] - dev[2][later]) > 1e-3 * c0[later])


def test_iteration_limit():
    opts = options(max_num_iterations=2, function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0)
    dev, _ = run_all(scene(7, models=MODELS), opts)
    assert (dev[0] == 1).all() and (dev[1] == 2).all()


def test_point_on_camera_centre_and_empty_view():
    P = scene(8, models=MODELS)
    # view 2: one more observation, of a point on its centre that only view 2 sees (code 3, untouched); view 5: no
    # observations (-1)
    P.points = np.vstack([P.points, np.r_[P.extrinsics[2, :3], 1.0]])
    P.point_constant = np.r_[P.point_constant, np.uint8(0)]
    P.obs_camera = np.r_[P.obs_camera, np.int32(2)]
    P.obs_point = np.r_[P.obs_point, np.int32(P.num_points - 1)]
    P.obs_xy = np.vstack([P.obs_xy, [500.0, 500.0]])
    keep = P.obs_camera != 5
    P.obs_camera, P.obs_point, P.obs_xy = P.obs_camera[keep], P.obs_point[keep], P.obs_xy[keep]
    dev, Pd = run_all(P, options())
    assert dev[0][2] == 3 and dev[0][5] == -1
    assert np.array_equal(Pd.extrinsics[[2, 5]], P.extrinsics[[2, 5]])


def test_summary_and_reproducibility():
    P = scene(9, models=MODELS)
    Pa, Pb = P.copy(), P.copy()
    a = lib.adjust_views(Pa, options())
    b = lib.adjust_views(Pb, options())
    for x, y in zip(a[:4], b[:4]):
        assert x.tobytes() == y.tobytes()
    assert Pa.extrinsics.tobytes() == Pb.extrinsics.tobytes()
    assert Pa.intrinsics.tobytes() == Pb.intrinsics.tobytes()
    term, iters, _, _, s = a
    assert s.num_views == (term >= 0).sum()
    assert s.num_success == ((term == 0) | (term == 1)).sum()
    assert s.total_iterations == iters[term >= 0].sum()
    assert s.num_chains == P.num_cameras
    assert s.seconds >= s.kernel_seconds > 0


def test_resident_form():
    """Solver.adjust_views on the resident parameters, then Solver.solve: the same as the one-shot batch followed by
    a one-shot solve, and as the oracle's sequence."""
    P = scene(10, models=MODELS)
    opts = options()
    S = lib.Solver(P.copy(), opts)
    dev = S.adjust_views(opts)
    Pl = P.copy()
    ref = sequential(Pl, opts)
    got = S.download().copy()
    check(dev, ref, got, Pl, "resident batch vs per-view device path")
    st, s = S.solve(opts)
    Po = P.copy()
    sequential(Po, opts, solver=oracle.solve)
    st_o, s_o = oracle.solve(Po, opts)
    assert st == st_o == 0 and s.num_iterations == s_o.num_iterations
    np.testing.assert_allclose(s.final_cost, s_o.final_cost, rtol=1e-9)
    S.close()


def test_resident_sharded_handle_refused():
    P = scene(11)
    S = lib.Solver(P, options(linear_solver_type=abi.ITERATIVE_SCHUR), rank=0, world=2)
    with pytest.raises(lib.EngineError) as e:
        S.adjust_views(options())
    assert e.value.status == 1  # TMI_BA_ERR_INVALID_ARGUMENT
    S.close()
