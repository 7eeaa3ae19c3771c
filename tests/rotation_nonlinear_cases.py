"""The inputs tests/test_gpu_rotation_nonlinear.py runs on the device, defined once so that
tests/test_rotation_nonlinear_cpu.py can hold the model to the conditions the comparison rests on (the decision margins,
the branches covered, MODEL_SPREAD) on exactly these inputs.

A case is a dict: gt [V, 3], view1, view2, rel [E, 3] (rotation_2), start [V, 3], view_given ([V] uint8 or None) and
options (overrides of the defaults, fixed_view among them).  Every shape comes twice: "<shape>, held" with
fixed_view >= 0, where the rotations themselves are compared, and "<shape>, free" with fixed_view = -1, the reference's
problem, where only gauge-invariant outputs are.

Graphs without a cycle (one edge, the path) and the star fit their measurements exactly, so a full solve drives the cost
to rounding, where neither the cost nor the function-tolerance test has any relative accuracy; those cases stop after
a few iterations, while the cost is still far above that.  In the free cases the LM diagonal A_ii / radius is all that
makes the gauge directions' pivots positive; every solve here ends within four iterations, at a radius below 1e6, so the
pivots' margins stay above the 1e-6 the comparison of decisions asks for (tests/test_rotation_nonlinear_cpu.py asserts it)
and no free case needs to be excused from it."""
import functools

import numpy as np

import rotation_nonlinear_model as model

# the free cases whose decisions are NOT compared with equality, with the model's margin (at most two; none is needed)
FREE_DECISIONS_NOT_COMPARED = {}


def _case(scene, held, options=None, start_noise=0.05, seed=0, view_given=None, start=None):
    gt, v1, v2, rel = scene
    if start is None:
        start = gt + start_noise * np.random.default_rng([seed, 7]).uniform(-1.0, 1.0, size=gt.shape)
    return dict(gt=gt, view1=v1, view2=v2, rel=rel, start=start, view_given=view_given, held=held,
                options=dict(options or {}))


def _shuffled_path(V, seed):
    """A chain through the views in a random order, its edges in a random order and direction."""
    rng = np.random.default_rng(seed)
    order = rng.permutation(V)
    pairs = [(int(order[i - 1]), int(order[i])) if rng.random() < 0.5 else (int(order[i]), int(order[i - 1]))
             for i in range(1, V)]
    return [pairs[i] for i in rng.permutation(len(pairs))]


def _star(leaves, seed):
    """A hub with `leaves` edges in both directions and 100 chords between the leaves."""
    pairs = [(0, i) if i % 2 else (i, 0) for i in range(1, leaves + 1)]
    rng = np.random.default_rng(seed)
    seen = set()
    while len(seen) < 100:
        a, b = (int(x) for x in rng.integers(1, leaves + 1, size=2))
        if a != b:
            seen.add((min(a, b), max(a, b)))
    return pairs + sorted(seen)


def _random(V, E, seed, noise=0.02, outliers=0.0):
    return model.scene_on_pairs(V, model.random_pairs(V, E, np.random.default_rng([seed, 1])), noise, seed, outliers)


def _measure(gt, v1, v2, noise, seed):
    """rotation_2 of the pairs for the ground truth `gt`, perturbed by up to `noise` radians."""
    err = noise * np.random.default_rng(seed).uniform(-1.0, 1.0, size=(v1.size, 3))
    return model.matrices_to_angle_axis(model.rotation_matrices(err) @ model.loop_rotations(gt, v1, v2))


def _zero_root():
    """View 0 starts at exactly zero, as the root of the spanning tree does, and its ground truth is zero too."""
    gt, v1, v2, _ = _random(10, 25, 71)
    gt = gt.copy()
    gt[0] = 0.0
    case = _case((gt, v1, v2, _measure(gt, v1, v2, 0.02, 73)), 0, seed=74)
    case["start"][0] = 0.0
    return case


def _unmarked():
    """Views 3 and 8 of 12 have no initialisation (their rows hold a sentinel that must come back bit for bit), and
    view 11 is marked but has edges to unmarked views only."""
    pairs = model.random_pairs(11, 28, np.random.default_rng([81, 1])) + [(11, 3), (8, 11)]
    case = _case(model.scene_on_pairs(12, pairs, 0.02, 81), 5, seed=82)
    given = np.ones(12, dtype=np.uint8)
    given[[3, 8]] = 0
    case["view_given"] = given
    case["start"][[3, 8]] = 1234.5
    return case


def _solution():
    """Every rotation and every relative rotation exactly zero: the start is the solution, the error rotation is exactly
    the identity (sin^2 = 0, the k = 2 branch) and the first gradient test ends the solve."""
    pairs = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 0), (0, 2)]
    v1 = np.array([p[0] for p in pairs], dtype=np.int32)
    v2 = np.array([p[1] for p in pairs], dtype=np.int32)
    z = np.zeros((5, 3))
    return _case((z, v1, v2, np.zeros((len(pairs), 3))), 2, start=z.copy())


def _mixed_solution():
    """The zero cluster of `_solution` inside a noisy graph: the k = 2 branch's Jacobian enters a real solve."""
    gt, v1, v2, _ = _random(9, 20, 91)
    gt = gt.copy()
    gt[:3] = 0.0
    rel = _measure(gt, v1, v2, 0.02, 92)
    inside = (v1 < 3) & (v2 < 3)
    assert inside.sum() >= 2
    rel[inside] = 0.0
    case = _case((gt, v1, v2, rel), 4, seed=93)
    case["start"][:3] = 0.0
    return case


_SHAPES = {
    "two views": lambda: _case(model.scene_on_pairs(2, [(0, 1)], 0.02, 11), 0, dict(max_num_iterations=1), seed=12),
    "two views (the last)": lambda: _case(model.scene_on_pairs(2, [(0, 1)], 0.02, 11), 1, dict(max_num_iterations=1),
                                          seed=12),
    "triangle": lambda: _case(model.scene_on_pairs(3, [(0, 1), (2, 1), (2, 0)], 0.02, 13), 1, seed=14),
    "22 views": lambda: _case(_random(22, 60, 21), 21, seed=22),
    "43 views": lambda: _case(_random(43, 120, 23), 0, seed=24),
    "shuffled path of 70": lambda: _case(model.scene_on_pairs(70, _shuffled_path(70, 31), 0.02, 32), 35,
                                         dict(max_num_iterations=3), seed=33),
    "star of 300": lambda: _case(model.scene_on_pairs(301, _star(300, 41), 0.02, 42), 17, dict(max_num_iterations=3),
                                 seed=43),
    "random 300/1500, a fifth outliers": lambda: _case(_random(300, 1500, 51, 0.02, 0.2), 150,
                                                       dict(max_num_iterations=12), seed=52),
    "zero-start root": _zero_root,
    "unmarked views": _unmarked,
    "given a solution": _solution,
    "a solution inside a noisy graph": _mixed_solution,
    "no iteration": lambda: _case(_random(8, 16, 61), 3, dict(max_num_iterations=0), seed=62),
    "one iteration": lambda: _case(_random(8, 16, 61), 3, dict(max_num_iterations=1), seed=62),
}


def _build(name):
    shape, mode = name.rsplit(", ", 1)
    case = _SHAPES[shape]()
    if mode == "held":
        case["options"]["fixed_view"] = case["held"]
    else:
        case["options"]["fixed_view"] = -1
    return case


HELD = [shape + ", held" for shape in _SHAPES]
FREE = [shape + ", free" for shape in _SHAPES]
CASES = HELD + FREE


@functools.lru_cache(maxsize=None)
def expected(name, path="own"):
    """(case, the model's result on `path`): computed once per case and shared; neither is modified by a test."""
    case = _build(name)
    return case, model.estimate(case["gt"].shape[0], case["view1"], case["view2"], case["rel"], case["start"],
                                case["view_given"], case["options"], path)


@functools.lru_cache(maxsize=None)
def model_spread(name):
    """MODEL_SPREAD of a free case: the largest gauge-invariant difference between the model's two linear-solve paths."""
    case, own = expected(name, "own")
    other = expected(name, "linalg")[1]
    return model.gauge_invariant_difference(own, other, case["view1"], case["view2"], used_views(case))


def used_views(case):
    given = np.ones(case["gt"].shape[0], dtype=bool) if case["view_given"] is None else case["view_given"].astype(bool)
    used = given[case["view1"]] & given[case["view2"]]
    return np.unique(np.concatenate([case["view1"][used], case["view2"][used]]))
