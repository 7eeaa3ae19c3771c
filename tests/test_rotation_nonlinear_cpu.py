"""tmi_ba_estimate_global_rotations_nonlinear without a device: the numpy model (tests/rotation_nonlinear_model.py)
against central differences at every branch of Ceres' rotation code, the loss and the corrector against a direct
evaluation, a noise-free recovery, the conditions the device comparison (tests/test_gpu_rotation_nonlinear.py) rests on --
the decision margins, MODEL_SPREAD, the branches covered -- on exactly the inputs that test uses
(tests/rotation_nonlinear_cases.py), the struct layouts, and the argument errors of the C ABI, which are refused before a
device is looked for."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402
import rotation_nonlinear_cases as cases  # noqa: E402
import rotation_nonlinear_model as model  # noqa: E402
from theiasfm_amd import abi, lib  # noqa: E402

INVALID_ARGUMENT, NO_DEVICE, UNSUPPORTED = 1, 2, 5
MIN_MARGIN = 1e-6


@pytest.fixture(scope="module")
def L():
    entry.build_engine()
    return lib.load()


# ---- the functor -------------------------------------------------------------------------------------------------------
def _branch_edges():
    """(x1, x2, rel, the code matrix_to_angle_axis must report) with every branch reachable by construction: generic
    edges; a zero view rotation on either side; an exactly zero error rotation; and outliers whose error rotation turns by
    2.8 radians (trace = 1 + 2 cos < 0) about an axis near each coordinate axis in turn, which makes that diagonal entry
    the largest, in both senses so that the quaternion's scalar part takes both signs."""
    rng = np.random.default_rng(3)
    x1 = rng.uniform(-1.0, 1.0, size=(12, 3))
    x2 = rng.uniform(-1.0, 1.0, size=(12, 3))
    x1[1] = 0.0
    x2[2] = 0.0
    loop = model.loop_rotations(np.vstack([x1, x2]), np.arange(12), np.arange(12, 24))
    err = 0.1 * rng.uniform(-1.0, 1.0, size=(12, 3))
    want = [0] * 12
    for i in range(3):
        for sign in (0, 1):
            axis = 0.05 * rng.uniform(-1.0, 1.0, size=3)
            axis[i] = 1.0
            err[4 + 2 * i + sign] = (2.8 if sign else -2.8) * axis / np.linalg.norm(axis)
            want[4 + 2 * i + sign] = None  # 1 + i, with or without the negative scalar part: checked below
    # rotation_2 = E^T (R2 R1^T), so that the error rotation R2 R1^T rotation_2^T is E
    rel = model.matrices_to_angle_axis(model.rotation_matrices(err).transpose(0, 2, 1) @ loop)
    x1[3] = x2[3] = rel[3] = 0.0  # all three exactly zero: the error rotation is exactly the identity
    want[3] = 4
    return x1, x2, rel, want, err


def test_functor_vanishes_on_consistent_rotations():
    rng = np.random.default_rng(1)
    gt = model.random_rotations(30, 1.5, rng)
    v1, v2 = rng.integers(0, 30, size=100), rng.integers(0, 30, size=100)
    rel = model.matrices_to_angle_axis(model.loop_rotations(gt, v1, v2))
    r = model.pairwise_rotation_error(gt[v1], gt[v2], rel)[0]
    assert np.abs(r).max() < 1e-14


def test_jacobian_against_central_differences_at_every_branch():
    x1, x2, rel, want, err = _branch_edges()
    r, J, (first1, first2, code) = model.pairwise_rotation_error(x1, x2, rel)
    assert first1.tolist() == [i in (1, 3) for i in range(12)] and first2.tolist() == [i in (2, 3) for i in range(12)]
    for e in range(12):
        if want[e] is not None:
            assert code[e] == want[e], e
    seen = set()
    for i in range(3):
        for sign in (0, 1):
            e = 4 + 2 * i + sign
            assert code[e] & 3 == 1 + i and not code[e] & 4, (e, code[e])
            seen.add(int(code[e]) >> 3)
            np.testing.assert_allclose(np.linalg.norm(r[e]), 2.8, rtol=1e-12)
    assert seen == {0, 1}  # the atan2(-sin, -cos) flip and its absence
    # the value is the error rotation that was built in (the outliers up to the sign of a rotation by more than pi / 2)
    np.testing.assert_allclose(model.rotation_matrices(r), model.rotation_matrices(err * (np.arange(12) != 3)[:, None]),
                               atol=1e-13)
    h = 1e-6
    for k in range(6):
        a, b = x1.copy(), x2.copy()
        (a if k < 3 else b)[:, k % 3] += h
        plus = model.pairwise_rotation_error(a, b, rel)[0]
        (a if k < 3 else b)[:, k % 3] -= 2.0 * h
        minus = model.pairwise_rotation_error(a, b, rel)[0]
        # central differences: h^2 |r'''| / 6 + eps |r| / h, about 1e-9 for these sizes
        np.testing.assert_allclose((plus - minus) / (2.0 * h), J[:, :, k], atol=2e-8, err_msg=str(k))


def test_soft_l_one_and_the_corrector_against_a_direct_evaluation():
    rng = np.random.default_rng(2)
    r = rng.uniform(-1.0, 1.0, size=(20, 3)) * np.logspace(-4, 0.4, 20)[:, None]
    J = rng.uniform(-1.0, 1.0, size=(20, 3, 6))
    a = 0.1
    s = (r * r).sum(axis=1)
    rho0, rho1, rho2 = model.soft_l_one(s, a)
    np.testing.assert_allclose(rho0, 2.0 * a * a * (np.sqrt(1.0 + s / (a * a)) - 1.0), rtol=1e-15)
    np.testing.assert_allclose(rho1, 1.0 / np.sqrt(1.0 + s / (a * a)), rtol=1e-15)
    np.testing.assert_allclose(rho2, -1.0 / (2.0 * a * a * (1.0 + s / (a * a)) ** 1.5), rtol=1e-14)
    # rho' is the derivative of rho (where s is large enough for sqrt(1 + s / b) - 1 to keep digits in a difference)
    big = s > 1e-3
    assert big.sum() >= 8
    h = 1e-5 * s[big]
    np.testing.assert_allclose((model.soft_l_one(s[big] + h, a)[0] - model.soft_l_one(s[big] - h, a)[0]) / (2.0 * h),
                               rho1[big], rtol=1e-7)
    assert (rho2 < 0.0).all()
    # the shortcut: |r~|^2 = rho' s, and J~^T r~ = rho' J^T r, the gradient of rho(s) / 2
    cost, rt, Jt = model.corrected(r, J, a)
    np.testing.assert_allclose((rt * rt).sum(axis=1), rho1 * s, rtol=1e-14)
    np.testing.assert_allclose(np.einsum("eki,ek->ei", Jt, rt), rho1[:, None] * np.einsum("eki,ek->ei", J, r), rtol=1e-13,
                               atol=1e-18)
    assert cost.tobytes() == rho0.tobytes()


@pytest.mark.parametrize("fixed_view", [-1, 4])
def test_noise_free_graph_is_recovered_up_to_gauge(fixed_view):
    rng = np.random.default_rng(5)
    gt, v1, v2, rel = model.scene_on_pairs(15, model.random_pairs(15, 40, rng), 0.0, 6)
    start = gt + 0.2 * rng.uniform(-1.0, 1.0, size=gt.shape)
    if fixed_view >= 0:
        start[fixed_view] = gt[fixed_view]
    out = model.estimate(15, v1, v2, rel, start, None, dict(fixed_view=fixed_view))
    assert out["termination"] == 0 and out["costs"][-1] < 1e-20
    assert model.aligned_rotation_difference(out["rotations"], gt, np.arange(15)) < 1e-9
    assert np.abs(model.loop_rotations(out["rotations"], v1, v2) - model.loop_rotations(gt, v1, v2)).max() < 1e-9
    if fixed_view >= 0:  # the gauge is held: the rotations themselves
        assert np.abs(model.rotation_matrices(out["rotations"]) - model.rotation_matrices(gt)).max() < 1e-9
        assert out["rotations"][fixed_view].tobytes() == gt[fixed_view].tobytes()


# ---- the conditions of the device comparison -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.HELD)
def test_no_decision_of_a_held_case_hinges_on_rounding(name):
    out = cases.expected(name)[1]
    print("%s: smallest decision margin %.3e over %d decisions" % (name, out["min_margin"], len(out["margins"])))
    assert out["min_margin"] > MIN_MARGIN


@pytest.mark.parametrize("name", cases.FREE)
def test_model_spread_of_a_free_case(name):
    """MODEL_SPREAD, and the margin that decides whether the device's decisions are compared with equality."""
    case, own = cases.expected(name)
    other = cases.expected(name, "linalg")[1]
    spread = cases.model_spread(name)
    print("%s: MODEL_SPREAD %.3e, smallest decision margin %.3e" % (name, spread, own["min_margin"]))
    assert spread < 1e-11  # two orders below the device tolerance's floor: 100 x MODEL_SPREAD stays at 1e-9
    if name in cases.FREE_DECISIONS_NOT_COMPARED:
        assert own["min_margin"] <= MIN_MARGIN
    else:
        assert own["min_margin"] > MIN_MARGIN
        assert own["outcomes"].tolist() == other["outcomes"].tolist()
        assert (own["iterations"], own["termination"], own["factorizations"]) == \
            (other["iterations"], other["termination"], other["factorizations"])
    assert len(cases.FREE_DECISIONS_NOT_COMPARED) <= 2


def test_the_cases_cover_every_branch_and_shape():
    seen = set()
    for name in cases.CASES:
        seen |= cases.expected(name)[1]["branches"]
    codes = {c for _, _, c in seen}
    assert {c & 3 for c in codes if not c & 4} == {0, 1, 2, 3}  # the trace and each largest diagonal entry
    assert any(c & 4 for c in codes) and any(c & 8 for c in codes)  # k = 2; the negative scalar part
    assert any(f1 for f1, _, _ in seen) and any(f2 for _, f2, _ in seen)  # the first-order matrix on either side
    orders = {name: 3 * (out["num_views"] - (name.endswith("held"))) for name in cases.CASES
              for out in [cases.expected(name)[1]]}
    assert orders["two views, free"] == 6 and orders["22 views, free"] == 66 and orders["43 views, free"] == 129
    assert orders["random 300/1500, a fifth outliers, free"] == 900
    case, out = cases.expected("unmarked views, held")
    skipped = np.isin(case["view1"], [3, 8]) | np.isin(case["view2"], [3, 8])
    assert skipped[-2:].all() and skipped.sum() > 2
    assert (out["num_views"], out["num_pairs"]) == (9, int((~skipped).sum()))  # 12 less 3 and 8, and 11 without an edge
    assert out["rotations"][[3, 8, 11]].tobytes() == case["start"][[3, 8, 11]].tobytes()
    assert (out["residuals"][skipped] == 0.0).all() and (out["residuals"][~skipped] != 0.0).any(axis=1).all()
    star = cases.expected("star of 300, held")[0]
    assert np.bincount(np.concatenate([star["view1"], star["view2"]]))[0] == 300  # longer than a workgroup


# ---- the C ABI without a device -------------------------------------------------------------------------------------------
def test_struct_layout_matches_header(tmp_path):
    O, S = abi.CNonlinearRotationOptions, abi.CNonlinearRotationSummary
    fields = [("tmi_ba_nonlinear_rotation_options", n) for n, _ in O._fields_] + \
             [("tmi_ba_nonlinear_rotation_summary", n) for n, _ in S._fields_]
    src = tmp_path / "sz.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "theia_mi355_ba.h"\nint main(){\n'
        'printf("%zu %zu\\n", sizeof(tmi_ba_nonlinear_rotation_options), sizeof(tmi_ba_nonlinear_rotation_summary));\n'
        + "".join(f'printf("%zu\\n", offsetof({t}, {n}));\n' for t, n in fields) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(O), C.sizeof(S)] + [getattr(O, n).offset for n, _ in O._fields_] + \
        [getattr(S, n).offset for n, _ in S._fields_]
    assert got == want


def test_options_init_matches_the_mirror(L):
    o = abi.CNonlinearRotationOptions()
    L.tmi_ba_nonlinear_rotation_options_init(C.byref(o))
    want = abi.nonlinear_rotation_options()
    for field, _ in abi.CNonlinearRotationOptions._fields_:
        assert getattr(o, field) == getattr(want, field) == model.DEFAULTS[field], field
    assert (o.max_num_iterations, o.robust_loss_width, o.fixed_view) == (200, 0.1, -1)
    with pytest.raises(AttributeError):
        abi.nonlinear_rotation_options(no_such_field=1)


def _call(L, batch, start, options=None, given=None, null=None):
    """The raw call with every optional output preset to 7: (status, every array as it was)."""
    o = options if options is not None else abi.nonlinear_rotation_options()
    k = max(int(o.max_num_iterations), 0) + 1
    rot = np.array(start, dtype=np.float64)
    outs = [np.full(k, 7.0), np.full(k, 7.0), np.full(k, 7, dtype=np.int32), np.full((max(batch.num_pairs, 1), 3), 7.0)]
    cb = batch.as_c()
    s = abi.CNonlinearRotationSummary()
    args = [C.byref(cb), C.byref(o), None if given is None else given.ctypes.data, -1, rot.ctypes.data] + \
        [a.ctypes.data for a in outs] + [C.byref(s)]
    if null is not None:
        args[null] = None
    rc = L.tmi_ba_estimate_global_rotations_nonlinear(*args)
    return rc, rot.tobytes() == np.asarray(start, dtype=np.float64).tobytes() and all((a == 7).all() for a in outs)


def _good():
    case = cases.expected("22 views, held")[0]
    return case, abi.ViewPairBatch(None, case["view1"], case["view2"], case["rel"], None, case["gt"].shape[0])


def test_the_two_refusals_and_every_invalid_argument_leave_the_outputs_untouched(L):
    case, good = _good()
    V, start = good.num_views, case["start"]
    assert _call(L, good, start) in ((0, False), (NO_DEVICE, True))
    # the reference's `false`: no constraint, no initialised view
    empty = abi.ViewPairBatch(None, case["view1"][:0], case["view2"][:0], case["rel"][:0], None, V)
    assert _call(L, empty, start) == (INVALID_ARGUMENT, True)
    assert b"no relative rotation" in L.tmi_ba_last_error()
    assert _call(L, good, start, given=np.zeros(V, dtype=np.uint8)) == (INVALID_ARGUMENT, True)
    assert b"no view has an initialisation" in L.tmi_ba_last_error()
    for null in (0, 1, 4, 9):  # batch, options, view_rotation, summary
        assert _call(L, good, start, null=null) == (INVALID_ARGUMENT, True), null

    def edit(a, i, value):
        a = a.copy()
        a[i] = value
        return a

    v1, v2, rel = good.pair_view1, good.pair_view2, good.pair_rotation2
    nan_rel = rel.copy()
    nan_rel[3, 1] = np.nan
    for why, batch in {
        "view index out of range": abi.ViewPairBatch(None, edit(v1, 2, V), v2, rel, None, V),
        "negative view index": abi.ViewPairBatch(None, v1, edit(v2, 2, -1), rel, None, V),
        "a view paired with itself": abi.ViewPairBatch(None, edit(v1, 5, v2[5]), v2, rel, None, V),
        "a repeated unordered pair": abi.ViewPairBatch(None, edit(v1, 7, v2[0]), edit(v2, 7, v1[0]), rel, None, V),
        "a non-finite rotation_2": abi.ViewPairBatch(None, v1, v2, nan_rel, None, V),
    }.items():
        assert _call(L, batch, start) == (INVALID_ARGUMENT, True), why
    for overrides in (dict(fixed_view=-2), dict(fixed_view=V), dict(robust_loss_width=0.0), dict(robust_loss_width=np.nan),
                      dict(robust_loss_width=np.inf), dict(max_num_iterations=-1), dict(function_tolerance=-1.0),
                      dict(initial_trust_region_radius=0.0), dict(min_lm_diagonal=np.nan)):
        assert _call(L, good, start, options=abi.nonlinear_rotation_options(**overrides)) == (INVALID_ARGUMENT, True), overrides
    given = np.ones(V, dtype=np.uint8)
    given[4] = 0
    assert _call(L, good, start, options=abi.nonlinear_rotation_options(fixed_view=4), given=given) == (INVALID_ARGUMENT, True)
    bad = start.copy()
    bad[4, 2] = np.nan
    assert _call(L, good, bad)[0] == INVALID_ARGUMENT
    # ... but an unmarked view's rotation is not read
    assert _call(L, good, bad, given=given)[0] in (0, NO_DEVICE)


def test_an_order_above_the_cap_is_refused(L, monkeypatch):
    case, good = _good()
    V = good.num_views
    held = abi.nonlinear_rotation_options(fixed_view=0)  # a held view takes three from the order
    monkeypatch.setenv("TMI_BA_ROTATION_MAX_ORDER", str(3 * V - 1))
    assert _call(L, good, case["start"]) == (UNSUPPORTED, True)
    assert _call(L, good, case["start"], options=held) in ((0, False), (NO_DEVICE, True))
    monkeypatch.setenv("TMI_BA_ROTATION_MAX_ORDER", str(3 * V - 4))
    assert _call(L, good, case["start"], options=held) == (UNSUPPORTED, True)
    monkeypatch.setenv("TMI_BA_ROTATION_MAX_ORDER", str(3 * V))
    assert _call(L, good, case["start"]) in ((0, False), (NO_DEVICE, True))
