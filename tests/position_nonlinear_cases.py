"""The inputs tests/test_gpu_position_nonlinear.py runs on the device, defined once so that
tests/test_position_nonlinear_cpu.py can hold the model to the conditions the comparison rests on (the reference's
bounds at the chosen seeds, the decision margins, the branches covered) on exactly these inputs.

A case is a dict: gt [V, 3] or None, view_rotation [V, 3], view1, view2, position_2 [E, 3], fixed_view, options (overrides
of the defaults, `seed` among them) and start ([V, 3] with positions_given, else None)."""
import functools

import numpy as np

import position_nonlinear_model as model

# Seeds at which the MODEL meets the reference's bounds (nonlinear_position_estimator_test.cc:259-282) from this
# project's start stream; tests/test_position_nonlinear_cpu.py asserts that, and the device test uses the same seeds.
REFERENCE_SCENE_SEED = 3
REFERENCE_START_SEED = {"reference 4/6 no noise": 1, "reference 4/6 1 degree": 1}
REFERENCE_BOUND = {"reference 4/6 no noise": 1e-4, "reference 4/6 1 degree": 0.1}  # squared error after alignment


def _case(scene, fixed=0, options=None, start=None):
    gt, o, v1, v2, p2 = scene
    return dict(gt=gt, view_rotation=o, view1=v1, view2=v2, position2=p2, fixed_view=fixed, options=dict(options or {}),
                start=start)


def _reference(name, noise):
    return _case(model.make_scene(4, 6, noise, REFERENCE_SCENE_SEED), 0, dict(seed=REFERENCE_START_SEED[name]))


def _shuffled_path(V, seed):
    """A chain through the views in a random order, its edges in a random order and direction."""
    rng = np.random.default_rng(seed)
    order = rng.permutation(V)
    pairs = [(int(order[i - 1]), int(order[i])) if rng.random() < 0.5 else (int(order[i]), int(order[i - 1]))
             for i in range(1, V)]
    pairs = [pairs[i] for i in rng.permutation(len(pairs))]
    return model.scene_on_pairs(V, pairs, 0.5, seed + 1)


def _star(leaves, seed):
    pairs = [(0, i) if i % 2 else (i, 0) for i in range(1, leaves + 1)]
    rng = np.random.default_rng(seed)
    seen = set()
    while len(seen) < 100:  # chords between the leaves, or the leaves' positions along their rays are free
        a, b = (int(x) for x in rng.integers(1, leaves + 1, size=2))
        if a != b:
            seen.add((min(a, b), max(a, b)))
    return model.scene_on_pairs(leaves + 1, pairs + sorted(seen), 0.5, seed + 1)


def _random_graph(V, E, seed, outliers):
    pairs = model.lud.random_pairs(V, E, np.random.default_rng([seed, 1]))
    return model.scene_on_pairs(V, pairs, 1.0, seed, outliers)


def _coincident():
    """positions_given, the two views of edge 4 (the chain's 4 - 5, away from the fixed view) start at the same point:
    the small-norm branch, Jacobian I."""
    scene = _random_graph(8, 16, 11, 0.0)
    gt, o, v1, v2, p2 = scene
    assert (int(v1[4]), int(v2[4])) == (4, 5)
    start = gt + 0.3 * np.random.default_rng(12).uniform(-1.0, 1.0, size=gt.shape)
    start[5] = start[4]
    return _case(scene, 0, dict(positions_given=1), start)


CASES = {
    "two views": lambda: _case(model.scene_on_pairs(2, [(0, 1)], 1.0, 5), 0, dict(seed=2)),
    "two views, the last fixed": lambda: _case(model.scene_on_pairs(2, [(0, 1)], 1.0, 5), 1, dict(seed=2)),
    "reference 4/6 no noise": lambda: _reference("reference 4/6 no noise", 0.0),
    "reference 4/6 1 degree": lambda: _reference("reference 4/6 1 degree", 1.0),
    "shuffled path of 70": lambda: _case(_shuffled_path(70, 31), 35, dict(seed=4, max_num_iterations=40)),
    "star of 300, hub fixed": lambda: _case(_star(300, 41), 0, dict(seed=5, max_num_iterations=25)),
    "star of 300, leaf fixed": lambda: _case(_star(300, 41), 17, dict(seed=5, max_num_iterations=25)),
    "random 40/200, a fifth outliers": lambda: _case(_random_graph(40, 200, 51, 0.2), 0, dict(seed=6, max_num_iterations=60)),
    "coincident start": _coincident,
    "fixed view first": lambda: _case(_random_graph(12, 30, 61, 0.0), 0, dict(seed=7)),
    "fixed view in the middle": lambda: _case(_random_graph(12, 30, 61, 0.0), 6, dict(seed=7)),
    "fixed view last": lambda: _case(_random_graph(12, 30, 61, 0.0), 11, dict(seed=7)),
    "no iteration": lambda: _case(model.make_scene(4, 6, 1.0, REFERENCE_SCENE_SEED), 0, dict(seed=1, max_num_iterations=0)),
    "one iteration": lambda: _case(model.make_scene(4, 6, 1.0, REFERENCE_SCENE_SEED), 0, dict(seed=1, max_num_iterations=1)),
}
PRE_ROTATED = ("random 40/200, a fifth outliers", "fixed view in the middle")  # run again with view_rotation NULL


@functools.lru_cache(maxsize=None)
def expected(name):
    """(case, the model's result): computed once per case and shared; neither is modified by a test."""
    case = CASES[name]()
    V = case["view_rotation"].shape[0]
    return case, model.estimate(V, case["view1"], case["view2"], case["position2"], case["view_rotation"],
                                case["fixed_view"], case["options"], case["start"])
