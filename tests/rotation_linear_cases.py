"""The inputs tests/test_gpu_rotation_linear.py runs on the device, defined once so that
tests/test_rotation_linear_cpu.py can hold the model (tests/rotation_linear_model.py) to the plain eigh answer and
record the margins on exactly these inputs.  Each is the smallest shape at which one part can go wrong.

A case is a dict: gt [V, 3] (or None), view1, view2, rel [E, 3] (rotation_2), given [V, 3] (what view_rotation holds on
entry: a sentinel, which the views without an edge must keep) and options (overrides of the defaults)."""
import functools

import numpy as np

import rotation_linear_model as model
from rotation_nonlinear_model import (loop_rotations, matrices_to_angle_axis, random_pairs, rotation_matrices,
                                      scene_on_pairs)
from rotation_nonlinear_cases import _shuffled_path, _star

SENTINEL = 1234.5
# the constant of model.derived_bound, chosen in tests/test_rotation_linear_cpu.py (the largest ratio observed for the
# model against the plain answer, with c = 1, is recorded there)
BOUND_C = 8.0
# the recorded seeds of "4 views, 1 degree" (tests/test_rotation_linear_cpu.py: the reflection branch)
SEED_ALL_REFLECTED = 2
SEED_NONE_REFLECTED = 0


def _case(scene, options=None, num_views=None):
    gt, v1, v2, rel = scene
    V = gt.shape[0] if num_views is None else num_views
    return dict(gt=gt, view1=np.asarray(v1, dtype=np.int32), view2=np.asarray(v2, dtype=np.int32),
                rel=np.ascontiguousarray(rel, dtype=np.float64), given=np.full((V, 3), SENTINEL), num_views=V,
                options=dict(options or {}))


def reference_scene(V, E, noise_degrees, seed):
    """The scene of linear_rotation_estimator_test.cc:139-180: orientations 0.2 x uniform(-1, 1)^3, the chain
    0-1-...-(V-1), then random pairs (first < second), rotation_2 = N R2 R1^T with N a rotation of exactly
    noise_degrees about a random axis."""
    rng = np.random.default_rng(seed)
    gt = 0.2 * rng.uniform(-1.0, 1.0, size=(V, 3))
    pairs = [(i - 1, i) for i in range(1, V)]
    seen = set(pairs)
    while len(pairs) < E:
        a, b = sorted(int(x) for x in rng.integers(0, V, size=2))
        if a != b and (a, b) not in seen:
            seen.add((a, b))
            pairs.append((a, b))
    v1 = np.array([p[0] for p in pairs], dtype=np.int32)
    v2 = np.array([p[1] for p in pairs], dtype=np.int32)
    axis = rng.normal(size=(len(pairs), 3))
    axis /= np.linalg.norm(axis, axis=1)[:, None]
    noise = rotation_matrices(np.deg2rad(noise_degrees) * axis)
    return gt, v1, v2, matrices_to_angle_axis(noise @ loop_rotations(gt, v1, v2))


def _random(V, E, seed, noise=0.02, outliers=0.0):
    return scene_on_pairs(V, random_pairs(V, E, np.random.default_rng([seed, 1])), noise, seed, outliers)


def _turntable():
    """36 views at 10 degree steps about one axis, each paired with the next two: sum R_i has rank 1."""
    V = 36
    gt = np.zeros((V, 3))
    gt[:, 1] = np.deg2rad(10.0) * np.arange(V) - np.pi + 0.05  # (angles in (-pi, pi))
    pairs = [(i, (i + 1) % V) for i in range(V)] + [((i + 2) % V, i) for i in range(V)]
    v1 = np.array([p[0] for p in pairs], dtype=np.int32)
    v2 = np.array([p[1] for p in pairs], dtype=np.int32)
    err = 0.01 * np.random.default_rng(61).uniform(-1.0, 1.0, size=(len(pairs), 3))
    return gt, v1, v2, matrices_to_angle_axis(rotation_matrices(err) @ loop_rotations(gt, v1, v2))


def _unused_indices():
    """15 view indices of which 3, 8 and 14 have no edge: they are not in the problem and are never written."""
    gt, v1, v2, rel = _random(12, 30, 71)
    where = np.array([i for i in range(15) if i not in (3, 8, 14)], dtype=np.int32)
    full = np.zeros((15, 3))
    full[where] = gt
    return full, where[v1], where[v2], rel


_CASES = {
    "2 views": lambda: _case(scene_on_pairs(2, [(1, 0)], 0.02, 11)),
    "4 views, noise-free": lambda: _case(reference_scene(4, 6, 0.0, 12)),
    "4 views, 1 degree": lambda: _case(reference_scene(4, 6, 1.0, 13)),
    "22 views": lambda: _case(_random(22, 60, 21)),
    "43 views": lambda: _case(_random(43, 120, 23)),
    "100 views / 800, 5 degrees": lambda: _case(reference_scene(100, 800, 5.0, 14)),
    "shuffled path of 70": lambda: _case(scene_on_pairs(70, _shuffled_path(70, 31), 0.02, 32)),
    "star of 300": lambda: _case(scene_on_pairs(301, _star(300, 41), 0.02, 42)),
    "turntable of 36": lambda: _case(_turntable()),
    "unused view indices": lambda: _case(_unused_indices()),
    "60 views / 300, a fifth outliers": lambda: _case(_random(60, 300, 51, 0.02, 0.2)),
    # (a tolerance its first iteration just misses: converged == 0 with a result the derived bound, which carries the
    # case's tolerance, still holds)
    "one iteration": lambda: _case(_random(8, 16, 61), dict(max_iterations=1, tolerance=5e-5)),
}
CASES = list(_CASES)
NOISE_FREE = "4 views, noise-free"
REFLECTION = "4 views, 1 degree"
# (case, the reference's bound in degrees against the ground truth after alignment by one rotation)
REFERENCE_TESTS = [("4 views, noise-free", 1e-6), ("4 views, 1 degree", 2.0), ("100 views / 800, 5 degrees", 5.0)]


@functools.lru_cache(maxsize=None)
def case(name):
    return _CASES[name]()


@functools.lru_cache(maxsize=None)
def expected(name, seed=None):
    """(case, the model's result): computed once per (case, seed) and shared; neither is modified by a test."""
    c = case(name)
    options = dict(c["options"])
    if seed is not None:
        options["seed"] = seed
    return c, model.estimate(c["num_views"], c["view1"], c["view2"], c["rel"], options, c["given"])


@functools.lru_cache(maxsize=None)
def plain(name):
    c = case(name)
    return model.plain(c["num_views"], c["view1"], c["view2"], c["rel"])


@functools.lru_cache(maxsize=None)
def probe_pairs(name):
    """The pairs on which loop rotations are compared: the case's edges and 50 random pairs of its views."""
    c = case(name)
    views = np.unique(np.concatenate([c["view1"], c["view2"]]))
    rng = np.random.default_rng(977)
    a, b = views[rng.integers(0, views.size, size=50)], views[rng.integers(0, views.size, size=50)]
    return np.concatenate([c["view1"], a]).astype(np.int64), np.concatenate([c["view2"], b]).astype(np.int64)


def bound(name, c=BOUND_C):
    """model.derived_bound of the case, with the case's tolerance, from eigh's eigenvalues (radians)."""
    k, p = case(name), plain(name)
    views = np.unique(np.concatenate([k["view1"], k["view2"]]))
    tol = k["options"].get("tolerance", model.DEFAULTS["tolerance"])
    return model.derived_bound(c, views.size, p["max_degree"], tol, p["eigenvalues"][3] - p["eigenvalues"][2])


def ritz_tolerance(name):
    """1e-9 x 2 maxdeg + the residual-over-gap term of the derived bound: what two runs of the same iteration may differ
    by in a Ritz value."""
    k, p = case(name), plain(name)
    n = 3 * np.unique(np.concatenate([k["view1"], k["view2"]])).size
    tol = k["options"].get("tolerance", model.DEFAULTS["tolerance"])
    scale = 2.0 * p["max_degree"]
    return 1e-9 * scale + (np.sqrt(3.0) * tol * scale + n * model.EPS * scale) / (p["eigenvalues"][3] - p["eigenvalues"][2])
