"""The inputs of the view-graph tests, defined once for the CPU and the GPU tests.  A case is a SimpleNamespace:
V, v1, v2 (int32), weight (int32, num_verified_matches), rotation2 [E, 3], mask (uint8 or None), root (-1: default) and
gt [V, 3], the orientations the noise-free relative rotations were made from (None where they were set by hand)."""
import functools
from types import SimpleNamespace

import numpy as np

import view_graph_model as model


def make(V, edges, weight=None, seed=0, mask=None, root=-1, rotation2=None):
    edges = np.asarray(edges, dtype=np.int32).reshape(-1, 2)
    E = edges.shape[0]
    gt = None
    if rotation2 is None:
        gt = np.random.default_rng(1000 + seed).uniform(-1.0, 1.0, size=(V, 3))  # (RandVector3d of the reference's test)
        if V:
            gt[0] = 0.0
        rotation2 = np.array([model.relative_rotation(gt[a], gt[b]) for a, b in edges]).reshape(E, 3)
    weight = np.full(E, 100, np.int32) if weight is None else np.asarray(weight, dtype=np.int32)
    return SimpleNamespace(V=int(V), v1=np.ascontiguousarray(edges[:, 0]), v2=np.ascontiguousarray(edges[:, 1]),
                           weight=weight, rotation2=np.asarray(rotation2, dtype=np.float64).reshape(E, 3),
                           mask=None if mask is None else np.asarray(mask, dtype=np.uint8), root=int(root), gt=gt)


def path_edges(order):
    return [(order[i], order[i + 1]) for i in range(len(order) - 1)]


def reference_scene(num_views, num_edges, seed):
    """CreateViewGraph of orientations_from_maximum_spanning_tree_test.cc:89-114: the path 0 - 1 - ... and random extra
    edges, every weight 100.  Edges are stored as ViewIdPairs (smaller view first), the rotation from the smaller."""
    rng = np.random.default_rng(seed)
    edges = path_edges(list(range(num_views)))
    have = set(edges)
    while len(edges) < num_edges:
        a, b = (int(x) for x in rng.choice(num_views, 2, replace=False))
        a, b = min(a, b), max(a, b)
        if (a, b) not in have:
            have.add((a, b))
            edges.append((a, b))
    return make(num_views, edges, seed=seed)


def _random_components(seed, views=2000, groups=40, isolated=100, extra=1.5):
    rng = np.random.default_rng(seed)
    name = rng.permutation(views)
    member = rng.integers(0, groups, size=views - isolated)
    edges = []
    for g in range(groups):
        vs = name[np.flatnonzero(member == g)]
        for i in range(1, len(vs)):
            edges.append((int(vs[i]), int(vs[rng.integers(0, i)])))  # a random tree: the group is connected
        for _ in range(int(extra * len(vs))):
            a, b = rng.choice(len(vs), 2, replace=False) if len(vs) > 1 else (0, 0)
            if a != b:
                edges.append((int(vs[a]), int(vs[b])))
    edges = [edges[i] for i in rng.permutation(len(edges))]
    return views, edges


def _star(leaves, hub):
    others = [v for v in range(leaves + 1) if v != hub]
    return [(hub, v) if i % 2 else (v, hub) for i, v in enumerate(others)]


def _two_components():
    """12 views: the largest component is {1, 3, 4, 6, 8, 9, 11}, the other {0, 2, 5, 7}; view 10 has no edge."""
    big = [(3, 1), (1, 4), (4, 6), (6, 3), (8, 6), (9, 8), (11, 9), (11, 1)]
    small = [(0, 2), (2, 5), (5, 7), (7, 0)]
    return 12, big + small, [50, 20, 30, 40, 10, 60, 70, 15, 90, 91, 92, 93]


@functools.lru_cache(maxsize=None)
def component_cases():
    rng = np.random.default_rng(5)
    perm300 = [int(x) for x in rng.permutation(300)]
    V, edges = _random_components(17)
    third = (np.random.default_rng(18).integers(0, 3, size=len(edges)) != 0).astype(np.uint8)
    nine = lambda e: make(9, e, rotation2=np.zeros((len(e), 3)))  # noqa: E731
    cases = {
        "one_view_no_edge": make(1, []),
        "single_edge": make(2, [(0, 1)]),
        "no_alive_edge": make(4, [(0, 1), (2, 3)], mask=[0, 0]),
        "equal_sizes_tie": make(7, [(4, 5), (5, 6), (2, 1), (2, 3)]),
        "reference_one_component": nine([(0, 1), (1, 2), (2, 3)]),
        "reference_two_components": nine([(0, 1), (1, 2), (2, 3), (5, 6), (6, 7)]),
        "reference_three_components": nine([(0, 1), (1, 2), (2, 3), (5, 6), (7, 8)]),
        "path_300_shuffled": make(300, path_edges(perm300), rotation2=np.zeros((299, 3))),
        "star_300": make(301, _star(300, 137), rotation2=np.zeros((300, 3))),
        "random_2000": make(V, edges, rotation2=np.zeros((len(edges), 3))),
        "random_2000_masked": make(V, edges, rotation2=np.zeros((len(edges), 3)), mask=third),
    }
    return cases


def _hand_rotations(kind, n):
    rng = np.random.default_rng(77)
    axes = rng.normal(size=(n, 3))
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    if kind == "zero":
        return np.zeros((n, 3))
    if kind == "tiny":
        return 1e-9 * axes
    return axes * (np.pi - 1e-6 * rng.uniform(0.0, 1.0, size=(n, 1)))  # within 1e-6 of pi


@functools.lru_cache(maxsize=None)
def tree_cases():
    rng = np.random.default_rng(9)
    k8 = [(a, b) for a in range(8) for b in range(a + 1, 8)]
    pairs12 = [(a, b) for a in range(12) for b in range(a + 1, 12)]
    distinct = [pairs12[i] for i in rng.permutation(len(pairs12))[:30]] + path_edges(list(range(12)))
    distinct = list(dict.fromkeys(distinct))
    order = list(range(300))
    perm300 = [int(x) for x in rng.permutation(300)]
    ties = set()
    while len(ties) < 3000 - 499:
        a, b = (int(x) for x in rng.choice(500, 2, replace=False))
        if abs(a - b) != 1:
            ties.add((min(a, b), max(a, b)))
    ties_edges = path_edges(list(range(500))) + sorted(ties)
    ties_edges = [ties_edges[i] if rng.integers(0, 2) else ties_edges[i][::-1] for i in rng.permutation(len(ties_edges))]
    V2, e2, w2 = _two_components()
    big = [1, 3, 4, 6, 8, 9, 11]
    wheel = path_edges(list(range(8))) + [(7, 0), (2, 6)]
    cases = {
        "k8_equal_weights": make(8, k8, seed=1),
        "distinct_weights": make(12, distinct, weight=rng.permutation(len(distinct)) + 1, seed=2),
        "cycle_lightest_left_out": make(6, [(0, 1), (1, 2), (3, 2), (3, 4), (5, 4), (5, 0)],
                                        weight=[7, 9, 3, 8, 6, 5], seed=3),
        "path_300_increasing": make(300, path_edges(order), weight=np.arange(1, 300), seed=4),
        "path_300_decreasing": make(300, path_edges(order), weight=np.arange(299, 0, -1), seed=5),
        "path_300_shuffled": make(300, path_edges(perm300), weight=np.arange(1, 300), seed=6),
        "star_hub_root": make(301, _star(300, 137), weight=rng.integers(1, 50, size=300), seed=7, root=137),
        "star_leaf_root": make(301, _star(300, 137), weight=rng.integers(1, 50, size=300), seed=7, root=300),
        "root_first": make(V2, e2, weight=w2, seed=8, root=big[0]),
        "root_middle": make(V2, e2, weight=w2, seed=8, root=big[3]),
        "root_last": make(V2, e2, weight=w2, seed=8, root=big[-1]),
        "root_default_masked": make(V2, e2, weight=w2, seed=8, mask=[1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1]),
        "ties_500_3000": make(500, ties_edges, weight=rng.integers(1, 6, size=len(ties_edges)), seed=10),
        "reference_4_6": reference_scene(4, 6, 150),
        "reference_50_100": reference_scene(50, 100, 151),
        "rotations_zero": make(8, wheel, rotation2=_hand_rotations("zero", len(wheel))),
        "rotations_1e-9": make(8, wheel, weight=np.arange(len(wheel), 0, -1), rotation2=_hand_rotations("tiny", len(wheel))),
        "rotations_near_pi": make(8, wheel, weight=np.arange(len(wheel), 0, -1), rotation2=_hand_rotations("pi", len(wheel))),
    }
    return cases


def root_outside_case():
    V2, e2, w2 = _two_components()
    return make(V2, e2, weight=w2, seed=8, root=5)


@functools.lru_cache(maxsize=None)
def component_model(name):
    c = component_cases()[name]
    return model.components(c.V, c.v1, c.v2, c.mask)


@functools.lru_cache(maxsize=None)
def tree_model(name):
    c = tree_cases()[name]
    return model.spanning_tree(c.V, c.v1, c.v2, c.weight, c.rotation2, c.mask, c.root)


def batch(case):
    """The case as an abi.ViewPairBatch of its own arrays (no view rotations: the view-graph calls do not read them)."""
    from theiasfm_amd import abi
    return abi.ViewPairBatch(None, case.v1.copy(), case.v2.copy(), case.rotation2.copy(), None, num_views=case.V)
