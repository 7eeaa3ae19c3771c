"""Batched two-view verification BA without a GPU: the CPU model (tests/two_view_verification_model.py) on constructed
pairs that reach every correspondence status, every pair status and both sides of the three gates; exact
correspondences of a true pose; the synthetic generator; the C ABI's struct layout, exports and argument checks."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as entry  # noqa: E402
import two_view_verification_model as model  # noqa: E402
from oracle import oracle  # noqa: E402
from theiasfm_amd import abi, lib, synth  # noqa: E402

MIN = 30
MODELS = [(abi.PINHOLE, 0.4), (abi.PINHOLE_RADIAL_TANGENTIAL, 0.15), (abi.FISHEYE, 0.15), (abi.FOV, 0.15),
          (abi.DIVISION_UNDISTORTION, 0.15)]
@pytest.fixture(scope="module")
def L():
    entry.build_engine()
    return lib.load()


def test_model_reaches_every_correspondence_status():
    rng = np.random.default_rng(1)
    side, kinds = model.mixed_pair(rng, 40, n_far=3, n_near=3, n_gross=2, n_behind=2)
    # a pair of cameras facing each other: the correspondence on the common axis has antiparallel rays, which pass the
    # angle test (dot = -1) and make the midpoint system singular (TriangulateMidpoint fails)
    Xf = model.points(rng, 40, (3.0, 7.0)) - [0.5, 0, 0, 0]
    Xf[7] = [0.0, 0.0, 5.0, 1.0]
    B = model.batch([side, model.pair(model.E2_FACING, Xf)])
    before = B.copy()
    out = model.verify(B, abi.two_view_verification_options())
    np.testing.assert_array_equal(out["correspondence_status"][:50], kinds)
    facing = out["correspondence_status"][50:]
    assert facing[7] == 2 and (np.delete(facing, 7) == 0).all()
    np.testing.assert_array_equal(out["pair_status"], [0, 0])
    np.testing.assert_array_equal(out["pair_num_verified"], [40, 39])
    assert set(out["termination"]) <= {0, 1}
    # points: written for the statuses 0 and 4 only
    wrote = np.isin(out["correspondence_status"], (0, 4))
    assert (B.points[wrote, 3] != 0).all() and (B.points[~wrote] == 0).all()
    # margins: the angle margin is finite for every tested correspondence, the near misses sit near no threshold
    assert np.isfinite(out["margin"]).all() and (out["margin"] > 1e-6).all()
    assert (out["margin_final"][wrote] > 1e-3).all()
    np.testing.assert_array_equal(B.extrinsics1, before.extrinsics1)
    np.testing.assert_array_equal(B.intrinsics1, before.intrinsics1)


@pytest.mark.parametrize("n_in,expect", [(MIN - 1, 1), (MIN, 1), (MIN + 1, 0)])
def test_model_input_gate(n_in, expect):
    """:171-176: BundleAdjustRelativePose is entered only with MORE than min_num_inlier_matches matches."""
    pair, _ = model.mixed_pair(np.random.default_rng(2), n_in)
    B = model.batch([pair])
    out = model.verify(B, abi.two_view_verification_options())
    assert out["pair_status"][0] == expect
    if expect == 1:
        assert (out["correspondence_status"] == -1).all() and (B.points == 0).all()
        assert out["termination"][0] == -1 and out["pair_num_verified"][0] == 0
    else:
        assert (out["correspondence_status"] == 0).all() and out["pair_num_verified"][0] == n_in


@pytest.mark.parametrize("n_in,expect", [(MIN - 1, 2), (MIN, 4), (MIN + 1, 0)])
def test_model_gate_after_triangulation(n_in, expect):
    """:268: FEWER than min survivors stop the pair; exactly min are adjusted (and then fail :181's `>`)."""
    pair, kinds = model.mixed_pair(np.random.default_rng(3), n_in, n_far=5)
    B = model.batch([pair])
    start = B.extrinsics2.copy()
    out = model.verify(B, abi.two_view_verification_options())
    assert out["pair_status"][0] == expect
    np.testing.assert_array_equal(out["correspondence_status"], kinds)
    assert out["pair_num_verified"][0] == n_in
    if expect == 2:
        assert out["termination"][0] == -1
        np.testing.assert_array_equal(B.extrinsics2, start)
    else:
        assert out["termination"][0] in (0, 1)


@pytest.mark.parametrize("n_in,expect", [(MIN - 1, 4), (MIN, 4), (MIN + 1, 0)])
def test_model_final_gate(n_in, expect):
    """:181: MORE than min verified matches; the three near misses survive the triangulation and fail the last filter."""
    pair, kinds = model.mixed_pair(np.random.default_rng(4), n_in, n_near=3)
    B = model.batch([pair])
    out = model.verify(B, abi.two_view_verification_options())
    np.testing.assert_array_equal(out["correspondence_status"], kinds)
    assert out["pair_status"][0] == expect and out["pair_num_verified"][0] == n_in
    assert out["termination"][0] in (0, 1)


def test_model_failed_adjustment_is_status_three():
    """model.failing_start_pair: a survivor whose triangulated point lies within 1e-4 of camera 1's centre fails the
    residual functor at the start point.  The solve ends with termination 3 and the pair with status 3 (:291-293): the
    correspondences keep the statuses of the triangulation, the points the triangulated values, the cameras and focal
    lengths are untouched.  The ordinary pair beside it is adjusted as usual."""
    rng = np.random.default_rng(5)
    side = model.noisy(model.mixed_pair(rng, 40)[0], rng)
    B = model.batch([model.failing_start_pair(rng), side])
    B.constant_intrinsics1[:] = 0  # free focal lengths: a write-back for the failed pair would show
    B.constant_intrinsics2[:] = 0
    T = B.copy()
    tri = model.verify(T, abi.two_view_verification_options(bundle_adjustment=0))
    assert (tri["correspondence_status"] == 0).all() and (tri["pair_status"] == 0).all()
    assert np.sum((T.points[3, :3] / T.points[3, 3] - B.extrinsics1[0, :3]) ** 2) < 1e-8
    before = B.copy()
    out = model.verify(B, abi.two_view_verification_options())
    np.testing.assert_array_equal(out["pair_status"], [3, 0])
    np.testing.assert_array_equal(out["termination"], [3, 0])
    assert out["iterations"][0] == 0 and out["pair_num_verified"][0] == 40
    np.testing.assert_array_equal(out["correspondence_status"], tri["correspondence_status"])
    np.testing.assert_array_equal(B.points[:40], T.points[:40])
    np.testing.assert_array_equal(B.extrinsics2[0], before.extrinsics2[0])
    np.testing.assert_array_equal(B.intrinsics1[0], before.intrinsics1[0])
    np.testing.assert_array_equal(B.intrinsics2[0], before.intrinsics2[0])
    assert (B.extrinsics2[1] != before.extrinsics2[1]).any()
    # max_num_iterations = 0 is NO_CONVERGENCE, which is usable: not a status 3
    one = model.batch([side])
    out = model.verify(one, abi.two_view_verification_options(), max_num_iterations=0)
    assert out["termination"][0] == 1 and out["iterations"][0] == 0 and out["pair_status"][0] == 0


def test_model_exact_correspondences_verify_and_keep_the_pose():
    B, truth = synth.make_two_view_verification_batch(6, 11, models=MODELS, pixel_noise=0.0, outlier_fraction=0.0,
                                                      roles=False, min_corr=60, max_corr=120)
    B.extrinsics2[:] = truth["extrinsics2"]
    out = model.verify(B, abi.two_view_verification_options())
    assert (out["correspondence_status"] == 0).all() and (out["pair_status"] == 0).all()
    np.testing.assert_array_equal(out["pair_num_verified"], np.diff(B.correspondence_ptr))
    assert np.abs(B.extrinsics2 - truth["extrinsics2"]).max() < 1e-8
    assert np.abs(B.points[:, :3] / B.points[:, 3:] - truth["points"][:, :3]).max() < 1e-6
    assert (out["final_cost"] < 1e-12).all()


def test_model_bundle_adjustment_off_stops_after_the_triangulation():
    B, _ = synth.make_two_view_verification_batch(14, 12, models=MODELS)
    A = B.copy()
    tri = model.verify(A, abi.two_view_verification_options(bundle_adjustment=0))
    assert set(tri["pair_status"]) == {0, 1, 2} and (tri["termination"] == -1).all()
    np.testing.assert_array_equal(A.extrinsics2, B.extrinsics2)
    full = model.verify(B, abi.two_view_verification_options())
    # the adjustment only turns 0 into 4
    changed = tri["correspondence_status"] != full["correspondence_status"]
    assert (tri["correspondence_status"][changed] == 0).all() and (full["correspondence_status"][changed] == 4).all()


def test_generator_roles_and_kinds():
    """synth.make_two_view_verification_batch: seeded, and its special pairs end where they are meant to."""
    B, truth = synth.make_two_view_verification_batch(20, 13, models=MODELS, free_intrinsics=0.3)
    B2, _ = synth.make_two_view_verification_batch(20, 13, models=MODELS, free_intrinsics=0.3)
    for f in ("extrinsics2", "intrinsics1", "intrinsics2", "features1", "features2", "correspondence_ptr", "model1"):
        np.testing.assert_array_equal(getattr(B, f), getattr(B2, f))
    assert (B.points == 0).all()
    n = np.diff(B.correspondence_ptr)
    role = truth["role"]
    assert [int(n[role.index(r)]) for r in ("gate1_min", "gate1_below", "gate1_tiny", "n63", "n64", "n65")] == \
        [MIN, MIN - 1, 3, 63, 64, 65]
    assert n[role.index("long")] >= 500 and set(truth["kind"]) == {0, 1, 2, 3, 4}
    out = model.verify(B, abi.two_view_verification_options())
    by_role = {r: int(out["pair_status"][p]) for p, r in enumerate(role) if r}
    assert by_role["gate1_min"] == 1 and by_role["gate1_below"] == 1 and by_role["gate1_tiny"] == 1
    assert by_role["gate2"] == 2
    assert by_role["end_min"] == 4 and out["pair_num_verified"][role.index("end_min")] == MIN
    assert by_role["end_min_plus_1"] == 0 and out["pair_num_verified"][role.index("end_min_plus_1")] == MIN + 1
    assert set(out["correspondence_status"]) == {-1, 0, 1, 3, 4}
    ordinary = np.array([r == "" for r in role])
    assert (out["pair_status"][ordinary] == 0).all()
    rejected = np.isin(out["correspondence_status"], (1, 2, 3, 4)).sum() / (out["correspondence_status"] >= 0).sum()
    assert 0.1 < rejected < 0.3


def test_model_in_permuted_order_agrees_with_itself():
    """The model on every pair's correspondences in another order: the triangulation is per correspondence, so its
    statuses and points are identical; after the adjustment (another summation order) a status may differ only where
    the model's own margin is below 1e-9."""
    B, _ = synth.make_two_view_verification_batch(16, 14, models=MODELS, free_intrinsics=0.3)
    Q, perm = model.permuted(B, np.random.default_rng(0))
    a = model.verify(B, abi.two_view_verification_options())
    b = model.verify(Q, abi.two_view_verification_options())
    differ = a["correspondence_status"][perm] != b["correspondence_status"]
    assert (np.minimum(a["margin_final"][perm], b["margin_final"])[differ] < 1e-9).all()
    assert differ.sum() <= 1e-3 * differ.size
    np.testing.assert_array_equal(a["margin"][perm], b["margin"])


# ---- the C ABI ----------------------------------------------------------------------------------
def test_symbols_are_exported(L):
    for name in ("tmi_ba_verify_two_views", "tmi_ba_two_view_verification_options_init"):
        assert name in lib.EXPORTS and hasattr(L, name)


def test_options_init_matches_the_python_defaults(L):
    o = abi.CTwoViewVerificationOptions()
    L.tmi_ba_two_view_verification_options_init(C.byref(o))
    d = abi.two_view_verification_options()
    for name, _ in abi.CTwoViewVerificationOptions._fields_:
        assert getattr(o, name) == getattr(d, name), name
    assert (o.min_num_inlier_matches, o.triangulation_max_reprojection_error, o.min_triangulation_angle_degrees,
            o.final_max_reprojection_error, o.bundle_adjustment) == (30, 15.0, 4.0, 5.0, 1)
    with pytest.raises(AttributeError):
        abi.two_view_verification_options(no_such_field=1)


def test_struct_layout_matches_header(tmp_path):
    O, S = abi.CTwoViewVerificationOptions, abi.CTwoViewVerificationSummary
    fields = [("tmi_ba_two_view_verification_options", n) for n, _ in O._fields_] + \
             [("tmi_ba_two_view_verification_summary", n) for n, _ in S._fields_]
    src = tmp_path / "sz.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "theia_mi355_ba.h"\nint main(){\n'
        'printf("%zu %zu\\n", sizeof(tmi_ba_two_view_verification_options), '
        "sizeof(tmi_ba_two_view_verification_summary));\n"
        + "".join(f'printf("%zu\\n", offsetof({t}, {n}));\n' for t, n in fields) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(O), C.sizeof(S)] + [getattr(O, n).offset for n, _ in O._fields_] + \
        [getattr(S, n).offset for n, _ in S._fields_]
    assert got == want


def _valid():
    B, _ = synth.make_two_view_verification_batch(3, 5, roles=False, min_corr=35, max_corr=40)
    return B


def _call(L, cb, options, point_dof=4, iters=200, summary=True):
    s = abi.CTwoViewVerificationSummary()
    return L.tmi_ba_verify_two_views(None if cb is None else C.byref(cb), None if options is None else C.byref(options),
                                     point_dof, iters, -1, None, None, None, None, None, None, None,
                                     C.byref(s) if summary else None)


def test_argument_errors_come_before_the_device(L):
    """Every one of these returns TMI_BA_ERR_INVALID_ARGUMENT (1), never TMI_BA_ERR_NO_DEVICE (2)."""
    nullp = lambda t: C.cast(None, C.POINTER(t))  # noqa: E731
    opts = abi.two_view_verification_options()
    B = _valid()
    assert _call(L, None, opts) == 1
    assert _call(L, B.as_c(), None) == 1
    assert _call(L, B.as_c(), opts, summary=False) == 1
    for dof in (0, 2, 5):
        assert _call(L, B.as_c(), opts, point_dof=dof) == 1
    assert _call(L, B.as_c(), opts, iters=-1) == 1
    assert _call(L, B.as_c(), abi.two_view_verification_options(min_num_inlier_matches=-1)) == 1
    cb = B.as_c()
    cb.num_pairs = -1
    assert _call(L, cb, opts) == 1
    for name, t in (("extrinsics1", C.c_double), ("extrinsics2", C.c_double), ("model1", C.c_int32),
                    ("model2", C.c_int32), ("intrinsics1", C.c_double), ("intrinsics2", C.c_double),
                    ("correspondence_ptr", C.c_int64), ("features1", C.c_double), ("features2", C.c_double),
                    ("points", C.c_double)):
        cb = B.as_c()
        setattr(cb, name, nullp(t))
        assert _call(L, cb, opts) == 1, name
    D = _valid()
    D.correspondence_ptr[1] = D.correspondence_ptr[2] + 1
    assert _call(L, D.as_c(), opts) == 1
    D = _valid()
    D.model2[1] = 5
    assert _call(L, D.as_c(), opts) == 1


def test_no_device_is_an_error_not_a_fallback(L):
    if L.tmi_ba_device_count() > 0:
        pytest.skip("a GPU is visible")
    B = _valid()
    before = B.copy()
    with pytest.raises(lib.EngineError) as e:
        lib.verify_two_views(B)
    assert e.value.args[0] == 2 or "2" in str(e.value)
    np.testing.assert_array_equal(B.extrinsics2, before.extrinsics2)
    np.testing.assert_array_equal(B.points, before.points)
