"""Seeded scenes for ExtractMaximallyParallelRigidSubgraph (tests/test_rigid_subgraph_cpu.py,
tests/test_gpu_rigid_subgraph.py).  The reference's random number generator is not reproduced: the scenes follow the
construction of extract_maximally_parallel_rigid_subgraph_test.cc:59-150 on numpy's.

Every scene is a dict: name, orientation [V, 3], view1 / view2 [E] int32, position2 [E, 3], view_mask ([V] uint8 or
None), options (overrides of the defaults) and, where the scene is built to show one, `expect`: null_dimension,
block_width, kept (the views with keep = 1), status.
"""
from __future__ import annotations

import functools

import numpy as np

import rigid_subgraph_model as model


def _poses(rng, num_views):
    """CreateViewsWithRandomPoses (:59-69): view 0 at the origin, the others uniform in [-1, 1]^3."""
    orientation = rng.uniform(-1.0, 1.0, (num_views, 3))
    position = rng.uniform(-1.0, 1.0, (num_views, 3))
    orientation[0] = 0.0
    position[0] = 0.0
    return orientation, position


def _position2(orientation, position, a, b):
    """CreateTwoViewInfo (:71-93): position_2 = R1 (c2 - c1) / |c2 - c1|."""
    t = position[b] - position[a]
    return model.angle_axis_to_rotation_matrix(orientation[a]) @ (t / np.linalg.norm(t))


def _random_unit(rng):
    v = rng.uniform(-1.0, 1.0, 3)
    return v / np.linalg.norm(v)


def _finish(name, orientation, edges, position2, view_mask=None, options=None, expect=None):
    """The edges in ascending (view1, view2), the order in which the shim hands over the reference's map."""
    order = sorted(range(len(edges)), key=lambda e: edges[e])
    return dict(name=name, orientation=np.ascontiguousarray(orientation),
                view1=np.array([edges[e][0] for e in order], dtype=np.int32),
                view2=np.array([edges[e][1] for e in order], dtype=np.int32),
                position2=np.array([position2[e] for e in order]).reshape(-1, 3),
                view_mask=None if view_mask is None else np.asarray(view_mask, dtype=np.uint8),
                options=dict(options or {}), expect=dict(expect or {}))


def reference_scene(name, seed, num_views, num_valid, num_invalid):
    """TestExtractMaximallyParallelRigidSubgraph (:152-171): a skeletal chain, random further valid pairs, then invalid
    pairs whose position_2 is a random unit vector (their rotation_2 += 1 is not read by this step)."""
    rng = np.random.default_rng(seed)
    orientation, position = _poses(rng, num_views)
    edges = [(i - 1, i) for i in range(1, num_views)]
    while len(edges) < num_valid:
        a, b = (int(x) for x in rng.permutation(num_views)[:2])
        if a > b or (a, b) in edges:
            continue
        edges.append((a, b))
    position2 = [_position2(orientation, position, a, b) for a, b in edges]
    while len(edges) < num_valid + num_invalid:
        a, b = (int(x) for x in rng.integers(0, num_views, 2))
        if a >= b or (a, b) in edges:
            continue
        edges.append((a, b))
        position2.append(_random_unit(rng))
    return _finish(name, orientation, edges, position2,
                   expect=dict(kept=list(range(num_views)), min_pairs_left=num_valid))


def core_with_leaves(seed=11, core=12, leaves=3):
    """(b) a rigid core (a chain and every second-neighbour pair, then random pairs) and `leaves` views hung on it by
    one edge each: every leaf can slide along its edge, so k = 4 + leaves, and no leaf is parallel to anything."""
    rng = np.random.default_rng(seed)
    V = core + leaves
    orientation, position = _poses(rng, V)
    edges = [(i - 1, i) for i in range(1, core)] + [(i - 2, i) for i in range(2, core)]
    while len(edges) < 3 * core:
        a, b = sorted(int(x) for x in rng.permutation(core)[:2])
        if (a, b) not in edges:
            edges.append((a, b))
    for leaf in range(leaves):
        edges.append((int(rng.integers(0, core)), core + leaf))
    position2 = [_position2(orientation, position, a, b) for a, b in edges]
    return _finish("core_with_leaves", orientation, edges, position2,
                   expect=dict(null_dimension=4 + leaves, block_width=8, kept=list(range(core))))


def chain(name, seed, num_views, options=None, expect=None):
    """A chain: every edge can stretch on its own, k = 3 + (V - 1), and no two views are parallel for any fixed view:
    every component has one view and the smallest view wins the tie."""
    rng = np.random.default_rng(seed)
    orientation, position = _poses(rng, num_views)
    edges = [(i - 1, i) for i in range(1, num_views)]
    position2 = [_position2(orientation, position, a, b) for a, b in edges]
    e = dict(null_dimension=num_views + 2)
    e.update(expect or {})
    return _finish(name, orientation, edges, position2, options=options, expect=e)


def isolated_and_masked(seed=23):
    """(e) ten views: view 2 has no edge, view 4 is outside the mask (its edges would make it part of the core); the
    other eight form a rigid graph."""
    rng = np.random.default_rng(seed)
    V = 10
    orientation, position = _poses(rng, V)
    live = [v for v in range(V) if v != 2]
    edges = [(a, b) for i, a in enumerate(live) for b in live[i + 1:i + 4]]
    position2 = [_position2(orientation, position, a, b) for a, b in edges]
    mask = np.ones(V, dtype=np.uint8)
    mask[4] = 0
    return _finish("isolated_and_masked", orientation, edges, position2, view_mask=mask,
                   expect=dict(null_dimension=4, block_width=8, kept=[v for v in live if v != 4]))


@functools.lru_cache(maxsize=None)
def scenes():
    """Every scene, built once.  (a) the reference's three tests, (b) core and leaves, (c) the chain whose null space
    fills the first block, (d) the chain that is refused, (e) isolated and masked views, and a chain long enough for the
    widest block (k = 64: widths 8, 16, 32, 64 are all null, 128 holds it)."""
    return (
        reference_scene("no_bad_rotations", 57, 10, 30, 0),
        reference_scene("few_bad_rotations", 58, 10, 30, 5),
        reference_scene("many_bad_rotations", 59, 30, 100, 30),
        core_with_leaves(),
        chain("chain6", 31, 6, expect=dict(block_width=16, kept=[0])),
        chain("chain12_refused", 32, 12, options=dict(max_null_dimension=8), expect=dict(status="NULL_SPACE_TOO_LARGE")),
        isolated_and_masked(),
        chain("chain62", 33, 62, expect=dict(block_width=128, kept=[0])),
    )


@functools.lru_cache(maxsize=None)
def model_spread():
    """MODEL_SPREAD: the largest entry of the difference of the two model paths' projectors N N^T over the scenes."""
    spread = 0.0
    for case in scenes():
        a, b = modelled(case["name"], "eigh")["null_space"], modelled(case["name"], "svd")["null_space"]
        spread = max(spread, float(np.abs(a @ a.T - b @ b.T).max()))
    return spread


@functools.lru_cache(maxsize=None)
def modelled(name, path="eigh"):
    """The model's answer for a scene, computed once and shared; treat it as read-only."""
    case = next(c for c in scenes() if c["name"] == name)
    return model.extract(case["orientation"], case["view1"], case["view2"], case["position2"], case["view_mask"], path=path)
