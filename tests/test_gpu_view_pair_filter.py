"""-m gpu: tmi_ba_filter_view_pairs_from_relative_translation and tmi_ba_filter_view_pairs_from_orientation
(view_pair_filter_kernels.h) against the CPU model (tests/view_pair_filter_model.py).

The ordering is a chain of single IEEE operations in a fixed order with fixed tie rules, so from identical
translations and axes the device's orders, bad weights and flags must equal the model's BYTES; only the rotation stage
and the orientation filter's angle (sincos, atan2) are compared through a tolerance, max(1e-15, 100 x MODEL_SPREAD),
where MODEL_SPREAD is the largest difference between two evaluations of the model itself."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import view_pair_filter_model as model  # noqa: E402
from theiasfm_amd import abi, lib, synth  # noqa: E402

pytestmark = pytest.mark.gpu

VIEW_COUNTS = (2, 3, 4, 10, 30, 63, 64, 65, 255, 256, 257, 300)
ITERATION_COUNTS = (1, 7, 48)


def _unit(a):
    return a / np.linalg.norm(a, axis=-1, keepdims=True)


def _axes(k, seed):
    return _unit(np.random.default_rng(1000 + seed).normal(size=(k, 3)))


def _path_graph(num_views, seed):
    """The path 0 - 1 - ... with about as many random chords in either orientation, in the global frame: the true
    direction of random positions, a third of them replaced by random unit vectors (so the graph has cycles the
    projections contradict)."""
    rng = np.random.default_rng(seed)
    V = num_views
    pos = rng.uniform(-1, 1, (V, 3))
    edges = {(i, i + 1) for i in range(V - 1)}
    pairs = [(i, i + 1) for i in range(V - 1)]
    want = min(2 * (V - 1), V * (V - 1) // 2)
    while len(pairs) < want:
        a, b = (int(x) for x in rng.choice(V, 2, replace=False))
        if (min(a, b), max(a, b)) in edges:
            continue
        edges.add((min(a, b), max(a, b)))
        pairs.append((a, b))
    e = np.asarray(pairs, np.int32)
    t = _unit(pos[e[:, 1]] - pos[e[:, 0]])
    bad = rng.random(len(e)) < 1.0 / 3.0
    t[bad] = _unit(rng.normal(size=(int(bad.sum()), 3)))
    return abi.ViewPairBatch(None, e[:, 0], e[:, 1], None, t, num_views=V)


def _device(B, axes, tolerance=0.08):
    o = abi.translation_filter_options(num_iterations=len(axes), translation_projection_tolerance=tolerance)
    return lib.filter_view_pairs_from_relative_translation(B, o, axes=axes)


def _model(B, axes, tolerance=0.08, translation=None):
    return model.filter_from_relative_translation(B.num_views, B.pair_view1, B.pair_view2, B.pair_position2, axes,
                                                  tolerance, translation=translation)


def _same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _check_exact(B, axes, tolerance=0.08):
    """Global-frame translations and given axes: orders, weights and flags equal the model's bytes."""
    removed, weight, rotated, order, used, fs = _device(B, axes, tolerance)
    m = _model(B, axes, tolerance)
    assert _same_bytes(used, np.asarray(axes, np.float64).reshape(-1, 3))
    assert _same_bytes(rotated, B.pair_position2)
    assert _same_bytes(order, m.order), np.argwhere(order != m.order)[:5]
    assert _same_bytes(weight, m.bad_weight), np.abs(weight - m.bad_weight).max()
    assert _same_bytes(removed, m.removed)
    degree = np.bincount(np.concatenate([B.pair_view1, B.pair_view2]), minlength=B.num_views)
    assert (fs.num_pairs, fs.num_pairs_removed, fs.num_iterations, fs.num_views_ordered) == \
        (B.num_pairs, int(m.removed.sum()), len(axes), int((degree > 0).sum()))
    return m


@pytest.mark.parametrize("iterations", ITERATION_COUNTS)
@pytest.mark.parametrize("views", VIEW_COUNTS)
def test_paths_with_chords_equal_the_model_bit_for_bit(views, iterations):
    B = _path_graph(views, views)
    m = _check_exact(B, _axes(iterations, views + iterations))
    if views >= 10:
        assert m.bad_weight.max() > 0  # (the case exercises the score rule, not only sources)


def test_bare_path():
    v = np.arange(70, dtype=np.int32)
    t = _unit(np.random.default_rng(5).normal(size=(69, 3)))
    m = _check_exact(abi.ViewPairBatch(None, v[:-1], v[1:], None, t, num_views=70), _axes(7, 5))
    assert (m.bad_weight == 0).all()  # a tree contradicts nothing


def test_star_with_a_hub_row_longer_than_the_workgroup():
    rng = np.random.default_rng(8)
    leaves = 300
    v1 = np.concatenate([np.zeros(leaves // 2), np.arange(leaves // 2 + 1, leaves + 1), np.arange(1, leaves)])
    v2 = np.concatenate([np.arange(1, leaves // 2 + 1), np.zeros(leaves - leaves // 2), np.arange(2, leaves + 1)])
    t = _unit(rng.normal(size=(len(v1), 3)))
    B = abi.ViewPairBatch(None, v1, v2, None, t, num_views=leaves + 1)
    assert np.bincount(B.pair_view1, minlength=1)[0] + np.bincount(B.pair_view2, minlength=1)[0] == leaves > 256
    assert _check_exact(B, _axes(7, 8)).bad_weight.max() > 0


def test_k12():
    rng = np.random.default_rng(12)
    pairs = [(a, b) if rng.random() < 0.5 else (b, a) for a in range(12) for b in range(a + 1, 12)]
    e = np.asarray(pairs, np.int32)
    B = abi.ViewPairBatch(None, e[:, 0], e[:, 1], None, _unit(rng.normal(size=(len(e), 3))), num_views=12)
    assert _check_exact(B, _axes(48, 12)).bad_weight.max() > 0


def test_two_components_and_isolated_views():
    rng = np.random.default_rng(3)
    a = [(0, 1), (1, 2), (2, 0), (2, 3), (3, 4), (4, 5), (6, 5), (6, 0)]
    b = [(8, 9), (9, 10), (10, 11), (11, 8), (12, 13), (13, 14), (14, 15), (15, 12), (11, 12)]
    e = np.asarray(a + b, np.int32)
    B = abi.ViewPairBatch(None, e[:, 0], e[:, 1], None, _unit(rng.normal(size=(len(e), 3))), num_views=20)
    m = _check_exact(B, _axes(7, 3))
    isolated = [7, 16, 17, 18, 19]
    assert (m.order[:, isolated] == -1).all() and (np.delete(m.order, isolated, axis=1) >= 0).all()
    assert (np.sort(np.delete(m.order, isolated, axis=1), axis=1) == np.arange(15)).all()


def test_every_translation_the_same_vector_ties_go_to_the_smallest_index():
    n = 40
    ring = [(i, (i + 1) % n) for i in range(n)]  # (n - 1, 0) closes a cycle of equal weights
    chords = [(5, 20), (31, 12), (7, 8 + 10), (25, 3)]
    e = np.asarray(ring + chords, np.int32)
    t = np.tile(_unit(np.array([0.3, -0.4, 0.5])), (len(e), 1))
    m = _check_exact(abi.ViewPairBatch(None, e[:, 0], e[:, 1], None, t, num_views=n), _axes(7, 40))
    ring_only = abi.ViewPairBatch(None, e[:n, 0], e[:n, 1], None, t[:n], num_views=n)
    m = _check_exact(ring_only, _axes(7, 41))
    for it, axis in enumerate(_axes(7, 41)):
        # view 0 wins the tie; after it the ring unwinds source by source, along the arcs' common direction
        forward = model.project(t[:1], axis)[0] > 0
        want = np.arange(n) if forward else np.concatenate([[0], np.arange(n - 1, 0, -1)])
        assert (m.order[it] == want).all()


def test_projections_that_are_exactly_zero():
    B = _path_graph(30, 77)
    B.pair_position2[:] = [1.0, 0.0, 0.0]
    axes = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, -1.0], [0.6, 0.8, 0.0], [0.0, 1.0, 0.0]])
    m = _check_exact(B, axes)
    assert (model.project(B.pair_position2, axes[0]) == 0.0).all() and (m.contribution[[0, 1, 3]] == 0.0).all()
    B = _path_graph(30, 78)
    B.pair_position2[::3] = [1.0, 0.0, 0.0]  # zero projections among the others
    B.pair_position2[1::3, 1] = 0.0
    _check_exact(B, axes)


_CHILD = """
import sys
import numpy as np
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import test_gpu_view_pair_filter as t
B = t._path_graph(300, 300)
removed, weight, rotated, order, used, fs = t._device(B, t._axes(7, 300))
np.savez({out!r}, removed=removed, weight=weight, order=order)
"""


def test_global_memory_state_equals_the_lds_state(tmp_path):
    """The 300-view graph again with TMI_BA_1DSFM_LDS_VIEWS=64 in a fresh process: the same body on the per-call
    global buffer gives the bytes of the LDS path."""
    B = _path_graph(300, 300)
    removed, weight, _, order, _, _ = _device(B, _axes(7, 300))
    out = str(tmp_path / "global_state.npz")
    env = dict(os.environ, TMI_BA_1DSFM_LDS_VIEWS="64")
    script = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), out=out)
    p = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    z = np.load(out)
    assert _same_bytes(z["order"], order) and _same_bytes(z["weight"], weight) and _same_bytes(z["removed"], removed)
    m = _model(B, _axes(7, 300))
    assert _same_bytes(z["order"], m.order) and _same_bytes(z["weight"], m.bad_weight)


def test_rotation_stage():
    B, _ = synth.make_view_pair_batch(30, 100, 30, 5)
    B.view_rotation[3] *= 1e-9  # the small-angle branch of AngleAxisRotatePoint
    axes = _axes(48, 5)
    removed, weight, rotated, order, _, _ = _device(B, axes)
    want, spread = model.rotate_translations(B.view_rotation, B.pair_view1, B.pair_position2)
    tol = max(1e-15, 100.0 * spread)
    err = float(np.abs(rotated - want).max())
    print(f"rotated_translation: device - model {err:.3e}, MODEL_SPREAD {spread:.3e}, tolerance {tol:.3e}")
    assert err <= tol
    # the ordering is discontinuous in its input: pinned from the device's own translations, not through a tolerance
    m = _model(B, axes, translation=rotated)
    assert _same_bytes(order, m.order) and _same_bytes(weight, m.bad_weight) and _same_bytes(removed, m.removed)


def test_drawn_axes():
    B, _ = synth.make_view_pair_batch(30, 100, 30, 6)
    o = abi.translation_filter_options(seed=17)
    removed, weight, rotated, order, axes, fs = lib.filter_view_pairs_from_relative_translation(B, o)
    assert axes.shape == (48, 3) and np.abs(np.linalg.norm(axes, axis=1) - 1.0).max() <= 1e-12
    again = lib.filter_view_pairs_from_relative_translation(B, abi.translation_filter_options(seed=17))
    assert all(_same_bytes(x, y) for x, y in zip(again[:5], (removed, weight, rotated, order, axes)))
    other = lib.filter_view_pairs_from_relative_translation(B, abi.translation_filter_options(seed=18))[4]
    assert np.abs(other - axes).max() > 1e-3
    assert len({tuple(a) for a in axes}) == 48  # 48 different axes
    m = _model(B, axes, translation=rotated)
    assert _same_bytes(order, m.order) and _same_bytes(weight, m.bad_weight) and _same_bytes(removed, m.removed)
    assert fs.num_pairs_removed == int(removed.sum()) and fs.kernel_seconds > 0 and fs.seconds >= fs.kernel_seconds


@pytest.mark.parametrize("seed", model.LINE_SEEDS)
def test_line_test_on_the_device(seed):
    V, v1, v2, pos = model.line_case()
    B = abi.ViewPairBatch(np.zeros((V, 3)), v1, v2, None, pos)
    removed = _device(B, model.draw_axes(pos, 48, seed), tolerance=0.1)[0]
    assert removed.tolist() == [0, 0, 0, 1]


@pytest.mark.parametrize("name,views,valid,invalid,seeds", model.REFERENCE_CASES, ids=[c[0] for c in model.REFERENCE_CASES])
def test_reference_cases_on_the_device(name, views, valid, invalid, seeds):
    for seed in seeds:
        B, _ = synth.make_view_pair_batch(views, valid, invalid, seed)
        t, _ = model.rotate_translations(B.view_rotation, B.pair_view1, B.pair_position2)
        removed = _device(B, model.draw_axes(t, 48, seed))[0]
        kept = int((removed == 0).sum())
        print(name, seed, "kept", kept, "of", B.num_pairs)
        assert kept >= valid, (name, seed)


def test_iterations_are_independent():
    B = _path_graph(30, 9)
    axes = _axes(48, 9)
    removed, weight, _, order, _, _ = _device(B, axes)
    total = np.zeros(B.num_pairs)
    for it in range(48):
        r1, w1, _, o1, _, _ = _device(B, axes[it:it + 1])
        assert _same_bytes(o1[0], order[it]), it
        total = total + w1
    assert _same_bytes(total, weight)
    assert _same_bytes(removed, (total > np.float64(0.08) * np.float64(48)).astype(np.uint8))


# ---- the orientation filter ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def orientation_scene():
    B, _ = synth.make_view_pair_batch(80, 1500, 500, 21)
    rng = np.random.default_rng(22)
    # valid edges off by up to 10 degrees, so that angles lie on both sides of the threshold
    B.pair_rotation2[:1500] += np.deg2rad(10.0) * rng.uniform(-0.6, 0.6, (1500, 3))
    angles, spread = model.loop_angles(B.view_rotation, B.pair_view1, B.pair_view2, B.pair_rotation2)
    return B, angles, spread


def test_orientation_filter_equals_the_model(orientation_scene):
    B, angles, spread = orientation_scene
    assert B.num_pairs == 2000
    degrees = 5.0
    threshold = degrees * (np.pi / 180.0)
    assert np.abs(angles - threshold).min() > 1e-9  # no edge at the threshold: decided on the CPU, from the model alone
    want = (angles * angles > threshold * threshold).astype(np.uint8)
    assert 200 < int(want[:1500].sum()) < 1300 and want[1500:].all()
    removed, got, fs = lib.filter_view_pairs_from_orientation(B, degrees)
    tol = max(1e-15, 100.0 * spread)
    err = float(np.abs(got - angles).max())
    print(f"pair_angle: device - model {err:.3e}, MODEL_SPREAD {spread:.3e}, tolerance {tol:.3e}")
    assert err <= tol
    assert _same_bytes(removed, want)
    assert (fs.num_pairs, fs.num_pairs_removed, fs.num_iterations) == (2000, int(want.sum()), 0)
    assert (got >= 0).all() and (got <= np.pi).all()


def test_orientation_filter_boundary_thresholds(orientation_scene):
    B, angles, _ = orientation_scene
    removed, got, fs = lib.filter_view_pairs_from_orientation(B, 180.0)
    assert not removed.any() and fs.num_pairs_removed == 0
    # threshold 0: everything with a positive angle goes.  An exactly consistent edge has an angle of round-off size,
    # zero or not, so the flags are held to the device's own angles and to the model where the model is clear.
    E = synth.make_view_pair_batch(20, 60, 10, 23)[0]
    model_angles, _ = model.loop_angles(E.view_rotation, E.pair_view1, E.pair_view2, E.pair_rotation2)
    removed, got, fs = lib.filter_view_pairs_from_orientation(E, 0.0)
    assert _same_bytes(removed, (got * got > 0.0).astype(np.uint8))
    assert removed[model_angles > 1e-9].all() and got[:60].max() < 1e-7
    assert fs.num_pairs_removed == int(removed.sum())
