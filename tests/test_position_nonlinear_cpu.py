"""tmi_ba_estimate_global_positions_nonlinear without a device: the numpy model (tests/position_nonlinear_model.py)
against a complex-step derivative of the reference's formula, the conditions the device comparison
(tests/test_gpu_position_nonlinear.py) rests on -- the reference's bounds at the chosen seeds, the decision margins, the
branches covered -- on exactly the inputs that test uses (tests/position_nonlinear_cases.py), and every argument error
of the C ABI, which is refused before a device is looked for."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402
import position_nonlinear_cases as cases  # noqa: E402
import position_nonlinear_model as model  # noqa: E402
from theiasfm_amd import abi, lib  # noqa: E402

INVALID_ARGUMENT, NO_DEVICE, UNSUPPORTED = 1, 2, 5
MIN_MARGIN = 1e-6


@pytest.fixture(scope="module")
def L():
    entry.build_engine()
    return lib.load()


# ---- the model's Jacobian and corrector ---------------------------------------------------------------------------------
def _edges():
    """Edges on both norm branches and both Huber branches (width 0.1): (p1, p2, t)."""
    rng = np.random.default_rng(1)
    p1 = rng.uniform(-5.0, 5.0, size=(8, 3))
    p2 = rng.uniform(-5.0, 5.0, size=(8, 3))
    u = (p2 - p1) / np.linalg.norm(p2 - p1, axis=1, keepdims=True)
    t = u.copy()
    t[:4] += 0.02 * rng.uniform(-1.0, 1.0, size=(4, 3))  # |r| <= 0.035: the quadratic branch
    t[4:] = rng.normal(size=(4, 3))                       # far off: the linear branch
    t[4:] /= np.linalg.norm(t[4:], axis=1, keepdims=True)
    p2[3] = p1[3]                                         # coincident: norm = 1, r = -t (linear branch)
    p2[7] = p1[7] + 1e-13                                 # below the tolerance as well
    return p1, p2, t


def test_jacobian_and_corrector_against_the_complex_step():
    p1, p2, t = _edges()
    r, _, norm, small = model.residuals(p1, p2, t)
    rho0, rho1, rho2, outer = model.huber((r * r).sum(axis=1), 0.1)
    assert small.tolist() == [False, False, False, True, False, False, False, True]
    assert outer[:3].tolist() == [False] * 3 and outer[3:].all()  # both Huber branches on both norm branches
    J2 = model.jacobian_analytic(p1, p2, t)
    np.testing.assert_allclose(J2, model.jacobian_complex_step(p1, p2, t, 2), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(-J2, model.jacobian_complex_step(p1, p2, t, 1), rtol=1e-12, atol=1e-15)
    assert (J2[small] == np.eye(3)).all()
    # the corrector: d(rho(|r|^2) / 2) / dp2 = J~^T r~ on both Huber branches, by the complex step on the cost itself
    _, rt, Jt, _ = model.corrected(r, J2, 0.1)
    grad = np.einsum("eki,ek->ei", Jt, rt)
    h = 1e-30
    for k in range(3):
        b = p2.astype(complex)
        b[:, k] += 1j * h
        rc = model.residuals(p1.astype(complex), b, t.astype(complex))[0]
        s = (rc * rc).sum(axis=1)
        cost = np.where(outer, 2.0 * 0.1 * np.sqrt(s) - 0.01, s) / 2.0
        np.testing.assert_allclose(grad[:, k], cost.imag / h, rtol=1e-12, atol=1e-15)
    # the values of HuberLoss on either side
    np.testing.assert_array_equal(rho1[~outer], 1.0)
    np.testing.assert_allclose(rho1[outer], 0.1 / np.sqrt((r * r).sum(axis=1))[outer], rtol=1e-15)
    assert (rho2[outer] < 0.0).all() and (rho2[~outer] == 0.0).all()


def test_start_stream_against_hand_computed_words():
    # splitmix64 from state 0: the first outputs of the published generator (Steele, Lea and Flood 2014; the test
    # vector of the reference implementation splitmix64.c)
    assert [model.splitmix64_word(0, c) for c in range(3)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    # from state 1234567: the vector of the same implementation
    assert [model.splitmix64_word(1234567, c) for c in range(2)] == [6457827717110365317, 3203168211198807973]
    start = model.start_positions(3, 0, fixed_view=1)
    u = ((0xE220A8397B1DCDAF >> 11) + 0.5) / 2.0 ** 53
    assert start[0, 0] == 100.0 * (2.0 * u - 1.0) and abs(start[0, 0] - 76.6621616427) < 1e-9
    assert (start[1] == 0.0).all() and (np.abs(start) < 100.0).all()
    u = ((model.splitmix64_word(0, 3 * 2 + 1) >> 11) + 0.5) / 2.0 ** 53
    assert start[2, 1] == 100.0 * (2.0 * u - 1.0)


# ---- the conditions of the device comparison, on the model --------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.REFERENCE_BOUND))
def test_reference_tests_through_the_model(name):
    """nonlinear_position_estimator_test.cc:259-282 at the seeds the device test uses."""
    case, res = cases.expected(name)
    err = float((model.aligned_errors(case["gt"], res["positions"]) ** 2).max())
    print("%s: largest squared error after alignment %.3e, %d iterations" % (name, err, res["iterations"]))
    assert res["termination"] == 0 and err < cases.REFERENCE_BOUND[name]


@pytest.mark.parametrize("name", list(cases.CASES))
def test_no_decision_of_the_model_hinges_on_rounding(name):
    case, res = cases.expected(name)
    print("%s: %d iterations, termination %d, smallest margin %.3e, outcomes %s" %
          (name, res["iterations"], res["termination"], res["min_margin"], res["outcomes"].tolist()))
    assert res["min_margin"] > MIN_MARGIN
    assert res["termination"] != 2 and len(res["outcomes"]) == res["iterations"] + 1
    assert np.isfinite(res["positions"]).all() and (res["positions"][case["fixed_view"]] == 0.0).all()
    assert (np.diff(res["costs"]) <= 0.0).all()  # an accepted step lowers the cost, any other keeps it


def test_the_cases_cover_every_branch():
    results = {name: cases.expected(name)[1] for name in cases.CASES}
    assert any(r["inner"] for r in results.values()) and any(r["outer"] for r in results.values())
    assert any((r["outcomes"] == 0).any() for r in results.values())  # a rejected step
    assert results["coincident start"]["small_norm"]
    assert not any(r["small_norm"] for name, r in results.items() if name != "coincident start")
    rejected = results["random 40/200, a fifth outliers"]
    assert rejected["outer"] and (rejected["outcomes"] == 0).any()
    assert results["no iteration"]["iterations"] == 0 and results["one iteration"]["iterations"] == 1
    assert {int(results[n]["termination"]) for n in results} == {0, 1}


# ---- the C ABI without a device -----------------------------------------------------------------------------------------
def _call(L, batch, fixed=0, options=None, start=None, null=None):
    """The raw call with every output preset to 7: (status, every output still 7)."""
    o = options if options is not None else abi.nonlinear_position_options()
    V, E = batch.num_views, batch.num_pairs
    k = max(int(o.max_num_iterations), 0) + 1
    pos = np.full((max(V, 1), 3), 7.0) if start is None else np.array(start, dtype=np.float64)
    before = pos.copy()
    outs = [np.full((max(V, 1), 3), 7.0), np.full(k, 7.0), np.full(k, 7.0), np.full(k, 7, dtype=np.int32),
            np.full((max(E, 1), 3), 7.0)]
    cb = batch.as_c()
    s = abi.CNonlinearPositionSummary()
    args = [C.byref(cb), C.byref(o), fixed, -1, pos.ctypes.data] + [a.ctypes.data for a in outs] + [C.byref(s)]
    if null is not None:
        args[null] = None
    rc = L.tmi_ba_estimate_global_positions_nonlinear(*args)
    untouched = pos.tobytes() == before.tobytes() and all((a == 7).all() for a in outs)
    return rc, untouched


def _batch(**changes):
    case = cases.CASES["fixed view first"]()
    parts = dict(o=case["view_rotation"], v1=case["view1"].copy(), v2=case["view2"].copy(), p2=case["position2"].copy(),
                 V=None)
    parts.update(changes)
    return abi.ViewPairBatch(parts["o"], parts["v1"], parts["v2"], None, parts["p2"], parts["V"])


def test_options_init_matches_the_mirror(L):
    o = abi.CNonlinearPositionOptions()
    L.tmi_ba_nonlinear_position_options_init(C.byref(o))
    want = abi.nonlinear_position_options()
    for field, _ in abi.CNonlinearPositionOptions._fields_:
        assert getattr(o, field) == getattr(want, field), field
        if field in model.DEFAULTS:
            assert getattr(o, field) == model.DEFAULTS[field], field
    assert (o.max_num_iterations, o.robust_loss_width) == (400, 0.1)  # nonlinear_position_estimator.h:71-72


def test_every_invalid_argument_is_refused_with_the_outputs_untouched(L):
    good = _batch()
    V, E = good.num_views, good.num_pairs
    # the arguments are fine: what is left is whether there is a device, and without one nothing is written
    assert _call(L, good) in ((0, False), (NO_DEVICE, True))
    for null in (0, 1, 4, 10):  # batch, options, view_position, summary
        assert _call(L, good, null=null) == (INVALID_ARGUMENT, True), null
    v1, v2 = good.pair_view1, good.pair_view2

    def edit(a, i, value):
        a = a.copy()
        a[i] = value
        return a

    nan_p2 = good.pair_position2.copy()
    nan_p2[3, 1] = np.nan
    inf_rot = good.view_rotation.copy()
    inf_rot[2, 0] = np.inf
    batches = {
        "view index out of range": _batch(v1=edit(v1, 2, V)),
        "negative view index": _batch(v2=edit(v2, 2, -1)),
        "a view paired with itself": _batch(v1=edit(v1, 5, v2[5])),
        "a repeated unordered pair": _batch(v1=edit(v1, 7, v2[0]), v2=edit(v2, 7, v1[0])),
        "a view not connected": abi.ViewPairBatch(np.vstack([good.view_rotation, np.zeros((1, 3))]), v1, v2, None,
                                                  good.pair_position2),
        "a non-finite position_2": _batch(p2=nan_p2),
        "a non-finite rotation": _batch(o=inf_rot),
        "no pair": abi.ViewPairBatch(good.view_rotation, v1[:0], v2[:0], None, good.pair_position2[:0]),
    }
    for why, batch in batches.items():
        assert _call(L, batch) == (INVALID_ARGUMENT, True), why
    for fixed in (-1, V):
        assert _call(L, good, fixed=fixed) == (INVALID_ARGUMENT, True), fixed
    for overrides in (dict(robust_loss_width=0.0), dict(robust_loss_width=-0.1), dict(robust_loss_width=np.nan),
                      dict(robust_loss_width=np.inf), dict(max_num_iterations=-1), dict(function_tolerance=-1.0),
                      dict(initial_trust_region_radius=0.0), dict(min_lm_diagonal=np.nan)):
        assert _call(L, good, options=abi.nonlinear_position_options(**overrides)) == (INVALID_ARGUMENT, True), overrides
    start = np.zeros((V, 3))
    start[4, 2] = np.nan
    assert _call(L, good, options=abi.nonlinear_position_options(positions_given=1), start=start) == (INVALID_ARGUMENT, True)
    assert b"non-finite position" in L.tmi_ba_last_error()
    assert E == 30


def test_an_order_above_the_cap_is_refused(L, monkeypatch):
    good = _batch()
    monkeypatch.setenv("TMI_BA_ROTATION_MAX_ORDER", str(3 * (good.num_views - 1) - 1))
    assert _call(L, good) == (UNSUPPORTED, True)
    # the cap comes before the connectivity check: a graph above it is refused whether connected or not
    apart = abi.ViewPairBatch(np.vstack([good.view_rotation, np.zeros((1, 3))]), good.pair_view1, good.pair_view2, None,
                              good.pair_position2)
    assert _call(L, apart) == (UNSUPPORTED, True)
    monkeypatch.setenv("TMI_BA_ROTATION_MAX_ORDER", str(3 * (good.num_views - 1)))
    rc, untouched = _call(L, good)
    assert (rc, untouched) in ((0, False), (NO_DEVICE, True))
