"""tmi_ba_estimate_global_positions_lud on the device against the numpy model (tests/position_lud_model.py).

The ADMM count and `converged` are compared exactly, on inputs for which the model's smallest decision margin exceeds
1e-6 (asserted first, on the CPU).  Positions and scales are compared as max |device - model| / max |model position|,
within max(1e-15, 100 x MODEL_SPREAD): MODEL_SPREAD is the largest difference, in the same measure, of the model from
its full-Cholesky, LU and permuted-numbering variants on the same input (DESIGN 8.7 has the figures observed).  The r / s
norm traces are compared with rtol 1e-9 and an absolute term for a vector of 4 E entries each off by the tolerance.
System orders 3 n sit at the tile (64) edges of the factorisation's pairs of panels and of the substitution.

With the reference's defaults ADMM reaches its stopping test on few of these inputs: on the model only order 3 and the
path (after one iteration, every scale exactly 1) and the reference's two 4 / 6 scenes (105 and 180 iterations) converge;
every other case runs to its iteration cap.  What is compared there is the trace and the iterate at the cap.  The order
cases (above order 3) take max_num_iterations = 200: what they are for, the tile edges, is exercised by the one
factorisation and by every substitution alike, and the path with chords, the middle fixed view, the reversed edges and
100 / 800 keep the default 1000 for what accumulates over a long loop.  The model runs four times per case (itself and
three variants for MODEL_SPREAD), once per session: under 1 s of numpy per 200 iterations, 2 to 3 s per 1000, 6 to 7 s
for 100 / 800; the device calls are a small part of the file's time.
Every scale is asserted >= 1 - 1e-2 on the model first and then on the device, converged or not: b = 1 on the scale rows
with z >= 0 holds s_e there from the first iterations on (the model's smallest over the cases is 0.9931, on the stars
after 30 iterations, and at least 0.9999 elsewhere)."""
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
import position_lud_model as model  # noqa: E402
from theiasfm_amd import abi, lib  # noqa: E402

pytestmark = pytest.mark.gpu
INVALID_ARGUMENT, UNSUPPORTED = 1, 5
MIN_MARGIN = 1e-6
REFERENCE_SEED = 3  # tests/test_position_lud_cpu.py asserts the reference's bounds on the model at this seed


@pytest.fixture(scope="module")
def L():
    entry.build_engine()
    return lib.load()


# ---- scenes: (ground truth, view_rotation or None, view1, view2, position_2, fixed_view, options or None) --------------
def _path(V):
    return [(i - 1, i) for i in range(1, V)]


def _chords(V, count, rng, have):
    out, seen = [], set((min(p), max(p)) for p in have)
    count = min(count, V * (V - 1) // 2 - len(seen))
    while len(out) < count:
        a, b = (int(x) for x in rng.integers(0, V, size=2))
        if a == b or (min(a, b), max(a, b)) in seen:
            continue
        seen.add((min(a, b), max(a, b)))
        out.append((a, b))  # (either direction)
    return out


def _scene(V, pairs, noise_deg, seed, fixed=0, options=None, outliers=0.0):
    gt, o, v1, v2, p2 = model.scene_on_pairs(V, pairs, noise_deg, seed, outliers)
    return gt, o, v1, v2, p2, fixed, options


def _order_case(V):
    pairs = _path(V)
    pairs += _chords(V, V, np.random.default_rng(100 + V), pairs)
    return _scene(V, pairs, 1.0, 200 + V, V // 2, dict(max_num_iterations=200) if V > 2 else None)


def _star(fixed):
    pairs = [(0, i) if i % 2 else (i, 0) for i in range(1, 300)]
    pairs += _chords(300, 80, np.random.default_rng(7), pairs)
    return _scene(300, pairs, 1.0, 8, fixed, dict(max_num_iterations=30))


def _reversed():
    pairs = _path(30) + _chords(30, 40, np.random.default_rng(5), _path(30))
    return _scene(30, [(max(p), min(p)) for p in pairs], 1.0, 25)


def _reference(views, pairs, noise, outliers=0.0):
    return model.make_scene(views, pairs, noise, REFERENCE_SEED, outliers) + (0, None)


CASES = {("order", 3 * (V - 1)): functools.partial(_order_case, V) for V in (2, 22, 23, 43, 44, 65, 66, 130)}
CASES.update({
    "two views, the first fixed": lambda: _scene(2, [(0, 1)], 1.0, 26),  # (("order", 3) fixes the last)
    "path": lambda: _scene(20, _path(20), 1.0, 21),
    "path with chords": lambda: _scene(40, _path(40) + _chords(40, 50, np.random.default_rng(3), _path(40)), 1.0, 22),
    "star, hub fixed": lambda: _star(0),
    "star, leaf fixed": lambda: _star(17),
    "fixed view in the middle": lambda: _scene(30, _path(30) + _chords(30, 40, np.random.default_rng(4), _path(30)), 1.0,
                                               24, 15),
    "reversed edges": _reversed,
    "reference 4/6 no noise": lambda: _reference(4, 6, 0.0),
    "reference 4/6 1 degree": lambda: _reference(4, 6, 1.0),
    "100/800 2 degrees, 10% outliers": lambda: _reference(100, 800, 2.0, 0.1),
})
REFERENCE_BOUND = {"reference 4/6 no noise": 1e-2, "reference 4/6 1 degree": 0.1}


@functools.lru_cache(maxsize=None)
def expected(name):
    """(scene, the model's result, MODEL_SPREAD): computed once per case and shared."""
    scene = CASES[name]()
    gt, o, v1, v2, p2, fixed, options = scene
    base = model.estimate(gt.shape[0], v1, v2, p2, o, fixed, options)
    return scene, base, model.model_spread(gt.shape[0], v1, v2, p2, o, fixed, options, base)


def _device(scene, pre_rotated=False):
    gt, o, v1, v2, p2, fixed, options = scene
    if pre_rotated:
        batch = abi.ViewPairBatch(None, v1, v2, None, model.directions(o, v1, p2), gt.shape[0])
    else:
        batch = abi.ViewPairBatch(o, v1, v2, None, p2)
    return lib.estimate_global_positions_lud(batch, fixed, abi.lud_position_options(**(options or {})))


def _compare(name, dev, base, spread):
    tol = max(1e-15, 100.0 * spread)
    scale = float(np.abs(base["positions"]).max())
    diff = model.difference(dev, base, scale)
    resid = float(np.abs(dev["residuals"] - base["residuals"]).max()) / scale
    print("%s: device difference %.3e (residuals %.3e), MODEL_SPREAD %.3e, tolerance %.3e, margin %.3e, ADMM %d%s" %
          (name, diff, resid, spread, tol, base["min_margin"], base["iterations"], "" if base["converged"] else " (cap)"))
    assert diff <= tol and resid <= tol
    return tol * scale


@pytest.mark.parametrize("name", list(CASES), ids=[str(k) for k in CASES])
def test_device_equals_model(L, name):
    scene, base, spread = expected(name)
    assert base["min_margin"] > MIN_MARGIN  # the trace is decided, not a matter of rounding
    gt, o, v1, v2, p2, fixed, options = scene
    dev = _device(scene)
    s = dev["summary"]
    absolute = _compare(name, dev, base, spread)
    assert (s.num_admm_iterations, bool(s.converged)) == (base["iterations"], base["converged"])
    assert s.num_factorizations == 1 and (s.num_views, s.num_pairs) == (gt.shape[0], v1.size)
    assert s.kernel_seconds > 0 and s.seconds >= s.kernel_seconds
    assert s.kernel_seconds == pytest.approx(s.factor_seconds + s.substitution_seconds + s.graph_seconds)
    atol = 1e-13 + absolute * np.sqrt(4.0 * v1.size)
    np.testing.assert_allclose(dev["r_norms"], base["r_norms"], rtol=1e-9, atol=atol)
    np.testing.assert_allclose(dev["s_norms"], base["s_norms"], rtol=1e-9, atol=opts_rho(options) * atol)
    assert (dev["positions"][fixed] == 0.0).all()
    print("%s: smallest scale on the model %.6f, on the device %.6f" % (name, base["scales"].min(), dev["scales"].min()))
    assert base["scales"].min() >= 1.0 - 1e-2  # b = 1 on the scale rows with z >= 0
    assert dev["scales"].min() >= 1.0 - 1e-2
    if name in REFERENCE_BOUND:  # the reference's own tests, after alignment to the ground truth
        for which, pos in (("model", base["positions"]), ("device", dev["positions"])):
            err = model.aligned_errors(gt, pos).max()
            print("%s: largest error after alignment on the %s %.3e" % (name, which, err))
            assert err < REFERENCE_BOUND[name]


def opts_rho(options):
    return (options or {}).get("rho", model.DEFAULTS["rho"])


def test_pre_rotated_directions_without_view_rotation(L):
    """view_rotation NULL with the model's t_e as position_2: the same problem without lud_direction_kernel."""
    for name in ("path with chords", ("order", 129)):
        scene, base, spread = expected(name)
        dev = _device(scene, pre_rotated=True)
        _compare(str(name) + " (pre-rotated)", dev, base, spread)
        assert (dev["summary"].num_admm_iterations, bool(dev["summary"].converged)) == (base["iterations"], base["converged"])


def test_two_calls_give_the_same_bits(L):
    for name in ("100/800 2 degrees, 10% outliers", "star, leaf fixed", ("order", 195)):
        scene = expected(name)[0]
        a, b = _device(scene), _device(scene)
        for key in ("positions", "scales", "residuals", "r_norms", "s_norms"):
            assert a[key].tobytes() == b[key].tobytes(), key
        assert a["summary"].num_admm_iterations == b["summary"].num_admm_iterations


def _raw(L, batch, fixed=0):
    cb = batch.as_c()
    o = abi.lud_position_options()
    s = abi.CLudPositionSummary()
    outs = [np.full((batch.num_views, 3), 7.0), np.full(batch.num_pairs, 7.0), np.full((batch.num_pairs, 3), 7.0),
            np.full(1000, 7.0), np.full(1000, 7.0)]
    rc = L.tmi_ba_estimate_global_positions_lud(C.byref(cb), C.byref(o), fixed, -1, *[a.ctypes.data for a in outs],
                                                C.byref(s))
    written = not any((a == 7.0).any() for a in outs[:3]) and not (outs[3][:s.num_admm_iterations] == 7.0).any()
    return rc, all((a == 7.0).all() for a in outs), written


def test_failures_leave_the_outputs_untouched(L, monkeypatch):
    gt, o, v1, v2, p2, fixed, _ = expected("path with chords")[0]
    V = gt.shape[0]
    # a view that nothing connects to the fixed one
    rc, untouched, _ = _raw(L, abi.ViewPairBatch(np.vstack([o, np.zeros((1, 3))]), v1, v2, None, p2))
    assert rc == INVALID_ARGUMENT and untouched
    # a non-finite input
    bad = p2.copy()
    bad[5, 1] = np.nan
    rc, untouched, _ = _raw(L, abi.ViewPairBatch(o, v1, v2, None, bad))
    assert rc == INVALID_ARGUMENT and untouched
    # an order above the (lowered) cap
    monkeypatch.setenv("TMI_BA_ROTATION_MAX_ORDER", str(3 * (V - 1) - 1))
    rc, untouched, _ = _raw(L, abi.ViewPairBatch(o, v1, v2, None, p2))
    assert rc == UNSUPPORTED and untouched
    monkeypatch.setenv("TMI_BA_ROTATION_MAX_ORDER", str(3 * (V - 1)))
    rc, untouched, written = _raw(L, abi.ViewPairBatch(o, v1, v2, None, p2), fixed=1)
    assert rc == 0 and not untouched and written
