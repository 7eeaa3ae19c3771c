"""tmi_ba_estimate_global_rotations_robust on the device against the numpy model (tests/robust_rotation_model.py).

The trace -- every ADMM count, the outer L1 count, the IRLS count -- is compared exactly, on inputs for which the model's
smallest decision margin exceeds 1e-6 (asserted first).  Rotations are compared as the angle of R_dev R_model^T per view
and the final residuals per edge, within max(1e-15, 100 x MODEL_SPREAD): MODEL_SPREAD is the larger of the model's
difference from its LU variant and from its permuted-numbering variant on the same input (DESIGN 8.6 has the figures
observed).  Orders n = V - 1 sit at the panel (32) and tile (64) edges of the Cholesky factorisation and of the
three-right-hand-side substitution."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402
import robust_rotation_model as model  # noqa: E402
from theiasfm_amd import abi, lib  # noqa: E402

pytestmark = pytest.mark.gpu
INVALID_ARGUMENT, UNSUPPORTED = 1, 5
MIN_MARGIN = 1e-6


@pytest.fixture(scope="module")
def L():
    entry.build_engine()
    return lib.load()


# ---- scenes -----------------------------------------------------------------------------------------------------------
def _path(V):
    return [(i - 1, i) for i in range(1, V)]


def _chords(V, count, rng, have):
    out, seen = [], set(have)
    while len(out) < count:
        a, b = (int(x) for x in rng.integers(0, V, size=2))
        if a == b or (min(a, b), max(a, b)) in seen:
            continue
        seen.add((min(a, b), max(a, b)))
        out.append((a, b))  # (either direction)
    return out


def _scene(V, pairs, noise_deg, seed, start_deg=3.0):
    """Ground truth 0.2 uniform(-1, 1)^3, relative rotations with noise, and a start start_deg away from the truth."""
    rng = np.random.default_rng(seed)
    gt = 0.2 * rng.uniform(-1.0, 1.0, size=(V, 3))
    v1 = np.array([p[0] for p in pairs], dtype=np.int32)
    v2 = np.array([p[1] for p in pairs], dtype=np.int32)
    rel = model.relative_rotation(gt[v1], gt[v2], noise_deg, rng)
    axis = rng.normal(size=(V, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    o0 = model.multiply_rotations(axis * np.deg2rad(start_deg), gt)
    return gt, v1, v2, rel, o0


def _order_case(n):
    V = n + 1
    rng = np.random.default_rng(100 + n)
    pairs = _path(V)
    pairs += _chords(V, min(V, V * (V - 1) // 2 - len(pairs)), rng, pairs)
    return _scene(V, pairs, 1.0, 200 + n) + (n // 2,)


def _star(fixed):
    rng = np.random.default_rng(7)
    pairs = [(0, i) if i % 2 else (i, 0) for i in range(1, 300)]
    pairs += _chords(300, 80, rng, [(0, i) for i in range(1, 300)])
    return _scene(300, pairs, 1.0, 8) + (fixed,)


def _duplicates():
    """every pair of a path with chords a second time, reversed with the inverse rotation and its own noise, and a few a
    third time in the first direction"""
    rng = np.random.default_rng(11)
    pairs = _path(20) + _chords(20, 15, rng, _path(20))
    gt, v1, v2, rel, o0 = _scene(20, pairs, 1.0, 12)
    rel_back = model.relative_rotation(gt[v2], gt[v1], 1.0, rng)
    rel_again = model.relative_rotation(gt[v1[:6]], gt[v2[:6]], 1.0, rng)
    return (gt, np.concatenate([v1, v2, v1[:6]]), np.concatenate([v2, v1, v2[:6]]),
            np.concatenate([rel, rel_back, rel_again]), o0, 4)


CASES = {("order", n): functools.partial(_order_case, n) for n in (1, 3, 31, 32, 33, 63, 64, 65, 129)}
CASES.update({
    "two views, the last fixed": lambda: _scene(2, [(0, 1)], 1.0, 25) + (1,),  # (("order", 1) fixes the first)
    "path": lambda: _scene(20, _path(20), 1.0, 21) + (0,),
    "path with chords": lambda: _scene(40, _path(40) + _chords(40, 50, np.random.default_rng(3), _path(40)), 1.0, 22) + (0,),
    "K12": lambda: _scene(12, [(a, b) for a in range(12) for b in range(a + 1, 12)], 1.0, 23) + (0,),
    "star, hub fixed": lambda: _star(0),
    "star, leaf fixed": lambda: _star(17),
    "duplicate edges": _duplicates,
    "fixed view in the middle": lambda: _scene(30, _path(30) + _chords(30, 40, np.random.default_rng(4), _path(30)), 1.0, 24) + (15,),
    "reference 4/6 no noise": lambda: model.make_scene(4, 6, 0.0, 0) + (0,),
    "reference 4/6 1 degree": lambda: model.make_scene(4, 6, 1.0, 0) + (0,),
    "reference 100/800 2 degrees": lambda: model.make_scene(100, 800, 2.0, 0) + (0,),
    "reference 100/800 2 degrees, 10% outliers": lambda: model.make_scene(100, 800, 2.0, 0, 0.1) + (0,),
})
REFERENCE_BOUND_DEG = {"reference 4/6 no noise": 1e-8, "reference 4/6 1 degree": 1.0, "reference 100/800 2 degrees": 5.0,
                       "reference 100/800 2 degrees, 10% outliers": 5.0}


@functools.lru_cache(maxsize=None)
def expected(name):
    """(scene, the model's result, MODEL_SPREAD): computed once per case and shared."""
    scene = CASES[name]()
    gt, v1, v2, rel, o0, fixed = scene
    base = model.estimate(gt.shape[0], v1, v2, rel, o0, fixed)
    return scene, base, model.model_spread(gt.shape[0], v1, v2, rel, o0, fixed, None, base)


def _device(scene, options=None):
    gt, v1, v2, rel, o0, fixed = scene
    return lib.estimate_global_rotations_robust(abi.RelativeRotationBatch(gt.shape[0], v1, v2, rel), o0, fixed, options)


def _compare(name, dev, base, spread):
    tol = max(1e-15, 100.0 * spread)
    angle = float(model.rotation_angles(dev["rotations"], base["rotations"]).max())
    resid = float(np.abs(dev["residuals"] - base["residuals"]).max())
    print("%s: rotation difference %.3e rad, residual difference %.3e, MODEL_SPREAD %.3e, tolerance %.3e, margin %.3e, "
          "ADMM %s, IRLS %d" % (name, angle, resid, spread, tol, base["min_margin"], base["admm_iterations"],
                                len(base["irls_steps"])))
    assert angle <= tol and resid <= tol
    return angle, resid


@pytest.mark.parametrize("name", list(CASES), ids=[str(k) for k in CASES])
def test_device_equals_model(L, name):
    scene, base, spread = expected(name)
    assert base["min_margin"] > MIN_MARGIN  # the trace is decided, not a matter of rounding
    dev = _device(scene)
    s = dev["summary"]
    assert dev["admm_iterations"] == base["admm_iterations"]
    assert s.num_l1_iterations == len(base["l1_steps"]) and s.num_irls_iterations == len(base["irls_steps"])
    assert s.num_admm_iterations == sum(base["admm_iterations"])
    assert (bool(s.l1_converged), bool(s.irls_converged)) == (base["l1_converged"], base["irls_converged"])
    assert s.num_factorizations == base["factorizations"]
    assert (s.num_views, s.num_pairs) == (scene[0].shape[0], scene[1].size)
    assert s.kernel_seconds > 0 and s.seconds >= s.kernel_seconds
    assert s.kernel_seconds == pytest.approx(s.factor_seconds + s.substitution_seconds + s.graph_seconds)
    _compare(name, dev, base, spread)
    np.testing.assert_allclose(dev["l1_steps"], base["l1_steps"], rtol=1e-9, atol=1e-13)
    np.testing.assert_allclose(dev["irls_steps"], base["irls_steps"], rtol=1e-9, atol=1e-13)
    np.testing.assert_allclose(dev["irls_sq_residuals"], base["irls_sq_residuals"], rtol=1e-9, atol=1e-13)
    fixed = scene[5]
    assert (dev["rotations"][fixed] == scene[4][fixed]).all()
    if name in REFERENCE_BOUND_DEG:  # the reference's own tests, after alignment to the ground truth
        for which, rot in (("model", base["rotations"]), ("device", dev["rotations"])):
            err = model.aligned_errors_deg(scene[0], rot).max()
            print("%s: largest error after alignment on the %s %.3e degrees" % (name, which, err))
            assert err < REFERENCE_BOUND_DEG[name]


def test_two_calls_give_the_same_bits(L):
    for name in ("reference 100/800 2 degrees, 10% outliers", "duplicate edges", "star, leaf fixed"):
        scene = expected(name)[0]
        a, b = _device(scene), _device(scene)
        assert a["rotations"].tobytes() == b["rotations"].tobytes()
        assert a["residuals"].tobytes() == b["residuals"].tobytes()
        assert a["admm_iterations"] == b["admm_iterations"]
        for key in ("l1_steps", "irls_steps", "irls_sq_residuals"):
            assert np.array(a[key]).tobytes() == np.array(b[key]).tobytes()


@pytest.mark.parametrize("name", [("order", 65), "duplicate edges", "star, hub fixed"], ids=str)
def test_one_irls_iteration_alone(L, name):
    """No L1 phase and one IRLS iteration: the weights, the assembly and the solve without the loops around them."""
    scene = expected(name)[0]
    gt, v1, v2, rel, o0, fixed = scene
    opt = dict(max_num_l1_iterations=0, max_num_irls_iterations=1)
    base = model.estimate(gt.shape[0], v1, v2, rel, o0, fixed, opt)
    spread = model.model_spread(gt.shape[0], v1, v2, rel, o0, fixed, opt, base)
    dev = _device(scene, abi.robust_rotation_options(**opt))
    s = dev["summary"]
    assert (s.num_l1_iterations, s.num_admm_iterations, s.num_irls_iterations, s.num_factorizations) == (0, 0, 1, 1)
    assert dev["admm_iterations"] == [] and len(dev["irls_steps"]) == 1
    _compare(str(name) + " (one IRLS iteration)", dev, base, spread)
    assert dev["irls_steps"][0] == pytest.approx(base["irls_steps"][0], rel=1e-9)


def _raw(L, batch, rot, fixed=0):
    cb = batch.as_c()
    o = abi.robust_rotation_options()
    s = abi.CRobustRotationSummary()
    res = np.full((batch.num_pairs, 3), 7.0)
    rc = L.tmi_ba_estimate_global_rotations_robust(C.byref(cb), C.byref(o), fixed, -1, rot.ctypes.data, res.ctypes.data,
                                                   None, None, None, None, C.byref(s))
    return rc, res


def test_failures_leave_the_orientations_untouched(L, monkeypatch):
    gt, v1, v2, rel, o0, fixed = expected("path with chords")[0]
    V = gt.shape[0]
    # a view that nothing connects to the fixed one
    lonely = abi.RelativeRotationBatch(V + 1, v1, v2, rel)
    rot = np.vstack([o0, np.zeros((1, 3))])
    before = rot.copy()
    rc, res = _raw(L, lonely, rot)
    assert rc == INVALID_ARGUMENT and (rot == before).all() and (res == 7.0).all()
    # a non-finite input
    bad = rel.copy()
    bad[5, 1] = np.nan
    rot = o0.copy()
    rc, res = _raw(L, abi.RelativeRotationBatch(V, v1, v2, bad), rot)
    assert rc == INVALID_ARGUMENT and (rot == o0).all() and (res == 7.0).all()
    # an order above the (lowered) cap
    monkeypatch.setenv("TMI_BA_ROTATION_MAX_ORDER", str(V - 2))
    rc, res = _raw(L, abi.RelativeRotationBatch(V, v1, v2, rel), rot)
    assert rc == UNSUPPORTED and (rot == o0).all() and (res == 7.0).all()
    monkeypatch.setenv("TMI_BA_ROTATION_MAX_ORDER", str(V - 1))
    rc, res = _raw(L, abi.RelativeRotationBatch(V, v1, v2, rel), rot)
    assert rc == 0 and not (rot == o0).all() and not (res == 7.0).any()
