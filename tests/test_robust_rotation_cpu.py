"""CPU checks of the rotation estimator: the numpy model (tests/robust_rotation_model.py) on the reference's three tests
(robust_rotation_estimator_test.cc:215-242), the decoupling identity A^T W A = L_w (x) I3 the device solve rests on, the
model's MultiplyRotations against scipy, and the C ABI's argument errors, which come before the device is looked for."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402
import robust_rotation_model as model  # noqa: E402
from theiasfm_amd import abi, lib  # noqa: E402

INVALID_ARGUMENT, NO_DEVICE, UNSUPPORTED = 1, 2, 5


@pytest.fixture(scope="module")
def L():
    entry.build_engine()
    return lib.load()


# ---- the reference's tests on the model -------------------------------------------------------------------------------
@pytest.mark.parametrize("views,pairs,noise,tolerance_deg", [(4, 6, 0.0, 1e-8), (4, 6, 1.0, 1.0), (100, 800, 2.0, 5.0)])
def test_reference_cases_on_the_model(views, pairs, noise, tolerance_deg):
    gt, v1, v2, rel, o0 = model.make_scene(views, pairs, noise, seed=0)
    res = model.estimate(views, v1, v2, rel, o0, 0)
    err = model.aligned_errors_deg(gt, res["rotations"])
    print("largest error after alignment: %.3e degrees; ADMM %s, IRLS %d" % (err.max(), res["admm_iterations"],
                                                                                len(res["irls_steps"])))
    assert err.max() < tolerance_deg
    assert (res["rotations"][0] == o0[0]).all()  # the fixed view keeps its value


def test_outliers_on_the_model():
    """100 / 800 / 2 degrees with 10 % of the edges replaced by random rotations still meets the 5 degree bound."""
    gt, v1, v2, rel, o0 = model.make_scene(100, 800, 2.0, seed=0, outlier_fraction=0.1)
    res = model.estimate(100, v1, v2, rel, o0, 0)
    assert model.aligned_errors_deg(gt, res["rotations"]).max() < 5.0


# ---- the decoupling identity ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixed", [0, 3, 6])
def test_normal_matrix_is_laplacian_kron_identity(fixed):
    """A^T W A built entry by entry as SetupLinearSystem (:101-147) and SolveIRLS (:198-208) build it equals
    L_w (x) I3 exactly; parallel and reversed edges included.  Weights are dyadic so that every sum is exact."""
    rng = np.random.default_rng(5)
    V = 7
    v1 = np.array([0, 1, 2, 3, 4, 5, 0, 2, 1, 6, 3, 0])
    v2 = np.array([1, 2, 3, 4, 5, 6, 3, 5, 0, 1, 0, 3])  # (0, 1) and (1, 0); (0, 3), (3, 0) and (0, 3) again
    E = v1.size
    w = rng.integers(1, 64, size=E) / 64.0
    g = model.Graph(V, v1, v2, fixed)
    A = np.zeros((3 * E, 3 * (V - 1)))
    for e in range(E):
        for k in range(3):
            if g.c1[e] >= 0:
                A[3 * e + k, 3 * g.c1[e] + k] = -1.0
            if g.c2[e] >= 0:
                A[3 * e + k, 3 * g.c2[e] + k] = 1.0
    at_weight = A.T * np.repeat(w, 3)[None, :]
    assert (at_weight @ A == np.kron(g.laplacian(w), np.eye(3))).all()
    assert (A.T @ A == np.kron(g.laplacian(), np.eye(3))).all()
    y = rng.integers(-8, 8, size=(E, 3)).astype(np.float64)
    assert (g.At(y).ravel() == A.T @ y.ravel()).all()
    x = rng.integers(-8, 8, size=(V - 1, 3)).astype(np.float64)
    assert (g.A(x).ravel() == A @ x.ravel()).all()


# ---- the model's pieces -----------------------------------------------------------------------------------------------
def test_multiply_rotations_against_scipy():
    rng = np.random.default_rng(2)
    a = rng.normal(size=(2000, 3))
    b = rng.normal(size=(2000, 3)) * np.array([0.01, 1.0, 2.0])[rng.integers(0, 3, size=2000), None]
    a[:5] = 0.0  # the first-order branch of AngleAxisToRotationMatrix
    b[5:10] = 1e-9
    got = model.multiply_rotations(a, b)
    want = (Rotation.from_rotvec(a) * Rotation.from_rotvec(b)).as_rotvec()
    # compare as rotations: near the angle pi the vector's sign is a matter of rounding
    assert model.rotation_angles(got, want).max() < 1e-14
    far = np.linalg.norm(want, axis=1) < 3.0
    assert np.abs(got[far] - want[far]).max() < 1e-13


def test_matrix_to_angle_axis_beyond_a_right_angle():
    """The branches of RotationMatrixToQuaternion for a negative trace (each diagonal entry the largest)."""
    for axis in np.eye(3):
        for angle in (2.2, 3.0, np.pi):
            aa = axis * angle
            back = model.matrix_to_angle_axis(model.angle_axis_to_matrix(aa))
            assert model.rotation_angles(back, aa).max() < 1e-14
            assert abs(np.linalg.norm(back) - angle) < 1e-13


def test_fixed_sum_is_a_sum():
    rng = np.random.default_rng(3)
    for n in (1, 255, 256, 257, 70000):
        x = rng.integers(-1000, 1000, size=n).astype(np.float64)
        assert model.fixed_sum(x) == x.sum()


def test_model_switches_agree_and_margins_are_recorded():
    gt, v1, v2, rel, o0 = model.make_scene(12, 30, 1.0, seed=4)
    base = model.estimate(12, v1, v2, rel, o0, 5)
    assert (base["rotations"][5] == o0[5]).all()
    decisions = 2 * sum(base["admm_iterations"]) + len(base["l1_steps"]) + len(base["irls_steps"])
    assert len(base["margins"]) == decisions and base["min_margin"] == min(base["margins"])
    spread = model.model_spread(12, v1, v2, rel, o0, 5, None, base)
    print("model spread", spread)
    assert spread < 1e-12


# ---- the ABI ----------------------------------------------------------------------------------------------------------
def test_symbols_and_defaults(L):
    for name in ("tmi_ba_robust_rotation_options_init", "tmi_ba_estimate_global_rotations_robust"):
        assert name in lib.EXPORTS and hasattr(L, name)
    o = abi.CRobustRotationOptions()
    L.tmi_ba_robust_rotation_options_init(C.byref(o))
    d = abi.robust_rotation_options()
    for name, _ in abi.CRobustRotationOptions._fields_:
        assert getattr(o, name) == getattr(d, name), name
    assert (o.max_num_l1_iterations, o.l1_step_convergence_threshold, o.max_num_irls_iterations,
            o.irls_step_convergence_threshold) == (5, 1e-3, 100, 1e-3)
    assert o.irls_loss_parameter_sigma == pytest.approx(np.deg2rad(5.0), rel=1e-15)


def _valid():
    gt, v1, v2, rel, o0 = model.make_scene(6, 9, 1.0, seed=1)
    return abi.RelativeRotationBatch(6, v1, v2, rel), o0


def _call(L, cb, rot, options=None, fixed=0, summary=True, batch=True, rotation=True):
    o = options if options is not None else abi.robust_rotation_options()
    s = abi.CRobustRotationSummary()
    return L.tmi_ba_estimate_global_rotations_robust(
        C.byref(cb) if batch else None, C.byref(o), fixed, -1, rot.ctypes.data if rotation else None, None, None, None,
        None, None, C.byref(s) if summary else None)


def _null(cb, name):
    setattr(cb, name, C.cast(None, type(getattr(cb, name))))


def _set(name, index, value):
    def edit(B, cb, rot):
        getattr(B, name).reshape(-1)[index] = value
    return edit


def _set_rotation(index, value):
    def edit(B, cb, rot):
        rot.reshape(-1)[index] = value
    return edit


def _disconnect(B, cb, rot):
    """view 5 loses its edges: every edge at it is rewired between views 0 and 1"""
    for e in range(B.num_pairs):
        if 5 in (B.pair_view1[e], B.pair_view2[e]):
            B.pair_view1[e], B.pair_view2[e] = 0, 1


BAD = {
    "negative num_views": lambda B, cb, rot: setattr(cb, "num_views", -1),
    "negative num_pairs": lambda B, cb, rot: setattr(cb, "num_pairs", -3),
    "no pairs": lambda B, cb, rot: setattr(cb, "num_pairs", 0),
    "no pair_view1": lambda B, cb, rot: _null(cb, "pair_view1"),
    "no pair_view2": lambda B, cb, rot: _null(cb, "pair_view2"),
    "no pair_rotation": lambda B, cb, rot: _null(cb, "pair_rotation"),
    "view index too large": _set("pair_view2", 1, 6),
    "view index negative": _set("pair_view1", 0, -1),
    "view paired with itself": _set("pair_view2", 2, 2),  # edge 2 is (2, 3)
    "non-finite relative rotation": _set("pair_rotation", 7, np.nan),
    "non-finite orientation": _set_rotation(4, np.inf),
    "a view not connected to the fixed one": _disconnect,
}


def test_argument_errors_come_before_the_device(L):
    """Each of these is TMI_BA_ERR_INVALID_ARGUMENT (1), never TMI_BA_ERR_NO_DEVICE (2), with a message, and the
    orientations are left alone."""
    def check(name, edit=None, **kw):
        B, rot = _valid()
        cb = B.as_c()
        if edit:
            edit(B, cb, rot)
        before = rot.copy()
        assert _call(L, cb, rot, **kw) == INVALID_ARGUMENT, name
        assert L.tmi_ba_last_error(), name
        assert np.array_equal(rot, before, equal_nan=True), name

    for name, edit in BAD.items():
        check(name, edit)
    for fixed in (-1, 6):
        check("fixed_view out of range", fixed=fixed)
    for field in ("l1_step_convergence_threshold", "irls_step_convergence_threshold", "irls_loss_parameter_sigma"):
        for value in (0.0, -1e-3, float("nan"), float("inf")):
            check(field, options=abi.robust_rotation_options(**{field: value}))
    for field in ("max_num_l1_iterations", "max_num_irls_iterations"):
        check(field, options=abi.robust_rotation_options(**{field: -1}))
    check("null batch", batch=False)
    check("null summary", summary=False)
    check("null view_rotation", rotation=False)


def test_order_above_the_cap_is_refused_before_the_device(L, monkeypatch):
    B, rot = _valid()
    monkeypatch.setenv("TMI_BA_ROTATION_MAX_ORDER", "4")  # n = 5
    before = rot.copy()
    assert _call(L, B.as_c(), rot) == UNSUPPORTED
    assert (rot == before).all() and b"cap" in L.tmi_ba_last_error()
    big = abi.RelativeRotationBatch(11002, np.arange(11001), np.arange(1, 11002), np.zeros((11001, 3)))
    monkeypatch.delenv("TMI_BA_ROTATION_MAX_ORDER")
    assert _call(L, big.as_c(), np.zeros((11002, 3))) == UNSUPPORTED


def test_a_valid_batch_reaches_the_device(L):
    """Without a device a valid batch is TMI_BA_ERR_NO_DEVICE (2) and nothing is written; with one it is OK."""
    want = 0 if L.tmi_ba_device_count() > 0 else NO_DEVICE
    B, rot = _valid()
    before = rot.copy()
    assert _call(L, B.as_c(), rot) == want
    # duplicate and reversed edges are valid here (unlike the view-pair filters' batch)
    D = abi.RelativeRotationBatch(6, np.concatenate([B.pair_view1, B.pair_view2[:2]]),
                                  np.concatenate([B.pair_view2, B.pair_view1[:2]]),
                                  np.concatenate([B.pair_rotation, -B.pair_rotation[:2]]))
    assert _call(L, D.as_c(), rot.copy(), fixed=3) == want
    assert _call(L, B.as_c(), rot.copy(), options=abi.robust_rotation_options(max_num_l1_iterations=0)) == want
    if want == NO_DEVICE:
        assert (rot == before).all()
        with pytest.raises(lib.EngineError) as e:
            lib.estimate_global_rotations_robust(B, rot)
        assert e.value.status == NO_DEVICE


def test_struct_layout_matches_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "theia_mi355_ba.h"\n'
        'int main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(tmi_ba_relative_rotation_batch),'
        "offsetof(tmi_ba_relative_rotation_batch, pair_rotation), sizeof(tmi_ba_robust_rotation_options),"
        "offsetof(tmi_ba_robust_rotation_options, max_num_irls_iterations),"
        "offsetof(tmi_ba_robust_rotation_options, irls_loss_parameter_sigma), sizeof(tmi_ba_robust_rotation_summary),"
        "offsetof(tmi_ba_robust_rotation_summary, num_factorizations),"
        "offsetof(tmi_ba_robust_rotation_summary, graph_seconds));return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    T, O, S = abi.CRelativeRotationBatch, abi.CRobustRotationOptions, abi.CRobustRotationSummary
    assert got == [C.sizeof(T), T.pair_rotation.offset, C.sizeof(O), O.max_num_irls_iterations.offset,
                   O.irls_loss_parameter_sigma.offset, C.sizeof(S), S.num_factorizations.offset, S.graph_seconds.offset]
