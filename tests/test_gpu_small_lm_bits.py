"""-m gpu: the four batched small-problem solvers (track, view, two-view and angular two-view LM kernels) return
the bits recorded in tests/golden/small_lm_bits.npz.  The goldens were written by tests/golden/make_small_lm_bits.py
before the trust-region loops were moved onto the shared core of small_lm.h; every output is compared with tobytes(),
so a change of rounding anywhere in a solver shows up here.

Covered: tmi_ba_adjust_views (PINHOLE at the default mask, mixed models with shared-intrinsics chains, HUBER, an
iteration limit), tmi_ba_adjust_two_views (point DOF 3 and 4, focal lengths constant and partly free, an iteration
limit), tmi_ba_adjust_two_views_angular,
tmi_ba_estimate_tracks (with and without track BA) and a small tmi_ba_solve with inner iterations (the third caller
of track_lm_kernel)."""
import os

import numpy as np
import pytest

from theiasfm_amd import abi, lib, synth

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "small_lm_bits.npz")
MIXED = [(abi.PINHOLE, 0.4), (abi.PINHOLE_RADIAL_TANGENTIAL, 0.15), (abi.FISHEYE, 0.15),
         (abi.FOV, 0.15), (abi.DIVISION_UNDISTORTION, 0.15)]


def options(**kw):
    kw.setdefault("linear_solver_type", abi.DENSE_QR)
    kw.setdefault("use_inner_iterations", 0)
    return abi.default_options(**kw)


def run_views():
    out = {}
    limit = dict(max_num_iterations=3, function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0)
    for name, models, share, kw in (("pinhole", None, 1, {}),
                                    ("mixed_chains", MIXED, 3, {}),
                                    ("huber", None, 1, dict(loss_function_type=abi.LOSS_HUBER)),
                                    ("mixed_limit", MIXED, 1, limit)):
        P = synth.make_problem(9, 200, 900, seed=61, scene="ring", spread=0.3, models=models,
                               shared_group_size=share, perturb=1.0)
        term, iters, c0, c1, _ = lib.adjust_views(P, options(**kw))
        out.update({f"views_{name}/{k}": v for k, v in (("term", term), ("iters", iters), ("c0", c0), ("c1", c1),
                                                        ("extrinsics", P.extrinsics), ("intrinsics", P.intrinsics))})
    return out


def run_two_views():
    out = {}
    for dof, free, limit in ((3, 0.0, 200), (3, 0.5, 200), (4, 0.0, 200), (4, 0.5, 200), (4, 0.5, 3)):
        B = synth.make_two_view_batch(12, 70 + dof, models=MIXED, free_intrinsics=free, max_corr=80)
        B.correspondence_ptr[-1] = B.correspondence_ptr[-2]  # a pair without correspondences
        term, iters, c0, c1, _ = lib.adjust_two_views(B, dof, max_num_iterations=limit)
        name = f"two_views_dof{dof}_free{int(free * 10)}_limit{limit}"
        out.update({f"{name}/{k}": v for k, v in (("term", term), ("iters", iters), ("c0", c0), ("c1", c1),
                                                  ("extrinsics2", B.extrinsics2), ("intrinsics1", B.intrinsics1),
                                                  ("intrinsics2", B.intrinsics2), ("points", B.points))})
    return out


def run_angular():
    B, _, _ = synth.make_two_view_angular_batch(24, 13, max_corr=60, noise=1e-3)
    ptr = B.correspondence_ptr.copy()
    ptr[5] = ptr[4]  # an empty pair
    B.correspondence_ptr = ptr
    term, iters, c0, c1, _ = lib.adjust_two_views_angular(B)
    return {f"angular/{k}": v for k, v in (("term", term), ("iters", iters), ("c0", c0), ("c1", c1),
                                           ("rotation2", B.rotation2), ("position2", B.position2))}


def run_estimate_tracks():
    out = {}
    for name, models, dof, ba in (("pinhole_dof3_ba", None, 3, 1), ("mixed_dof4_ba", MIXED, 4, 1),
                                  ("mixed_dof4_noba", MIXED, 4, 0)):
        P = synth.make_problem(10, 300, 1400, seed=83, scene="ring", spread=0.3, models=models, perturb=0.2)
        rng = np.random.default_rng(84)
        bad = rng.random(P.num_observations) < 0.03
        P.obs_xy[bad] += rng.normal(0, 30.0, (int(bad.sum()), 2))
        P.points[:] = rng.normal(0, 50.0, P.points.shape)  # ignored: every selected track is triangulated anew
        status, _ = lib.estimate_tracks(P, abi.track_estimator_options(bundle_adjustment=ba),
                                        options(point_dof=dof))
        out[f"estimate_{name}/status"] = status
        out[f"estimate_{name}/points"] = P.points
    return out


def run_inner():
    out = {}
    for name, models, dof, loss in (("pinhole_dof3", None, 3, abi.LOSS_TRIVIAL),
                                    ("mixed_dof4_huber", MIXED, 4, abi.LOSS_HUBER)):
        P = synth.make_problem(8, 250, 1200, seed=97, scene="ring", spread=0.3, models=models)
        st, s = lib.solve(P, abi.default_options(point_dof=dof, loss_function_type=loss,
                                                 linear_solver_type=abi.DENSE_SCHUR, max_num_iterations=6,
                                                 use_inner_iterations=1))
        assert st == 0
        summary = np.array([s.initial_cost, s.final_cost])
        counts = np.array([s.num_iterations, s.num_successful_steps, s.num_inner_iteration_steps], dtype=np.int32)
        out.update({f"inner_{name}/{k}": v for k, v in (("costs", summary), ("counts", counts),
                                                        ("extrinsics", P.extrinsics), ("intrinsics", P.intrinsics),
                                                        ("points", P.points))})
    return out


RUNS = {"views": run_views, "two_views": run_two_views, "angular": run_angular,
        "estimate_tracks": run_estimate_tracks, "inner": run_inner}


@pytest.mark.parametrize("what", list(RUNS))
def test_small_lm_bits_unchanged(what):
    g = np.load(GOLDEN)
    got = RUNS[what]()
    assert got and all(k in g.files for k in got), what
    for key, val in got.items():
        ref = g[key]
        assert val.dtype == ref.dtype and val.shape == ref.shape, key
        assert val.tobytes() == ref.tobytes(), key
