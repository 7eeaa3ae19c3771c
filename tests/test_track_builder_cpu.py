"""tmi_ba_build_tracks without a device: the model of tests/track_builder_model.py (the reference's loop) on the
reference's five tests, step 3's argument -- the reference's loop over ALL edges equals "unconstrained components, then
a replay per oversize component" -- checked in numpy on random graphs, and the contents of the random inputs the GPU
tests use."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_builder_model as model  # noqa: E402


def test_model_on_the_reference_tests():
    got = []
    for name, ev, ef, min_len, max_len, expected in model.reference_cases():
        r = model.build_tracks(ev, ef, min_len, max_len)
        got.append(r["num_tracks"])
        assert r["num_tracks"] == expected, name
        assert r["num_sets"] == r["num_tracks"] + r["num_small_tracks"]
        # VerifyTracks: a track names a view once
        for t in range(r["num_tracks"]):
            views = r["obs_view"][r["track_begin"][t]:r["track_begin"][t + 1]]
            assert len(set(views.tolist())) == len(views) >= max(min_len, 2)
    assert got == [4, 1, 2, 3, 1]


def components_then_replay(endpoint_node, num_nodes, max_track_length):
    """Step 3 as the ABI comment states it, on its own: the components with no cap; a component within the cap is one
    set; a larger one has its own edges replayed in ascending edge index on a LOCAL numbering, the smaller root
    surviving (the reference unites by size: only the partition matters).  Returns the label of every node."""
    node = np.asarray(endpoint_node, dtype=np.int64)
    comp = model.unconstrained_components(node, num_nodes)
    size = np.bincount(comp, minlength=num_nodes)
    label = comp.copy()
    edge_comp = comp[node[0::2]]
    assert np.array_equal(edge_comp, comp[node[1::2]])
    for c in np.flatnonzero(size > max_track_length):
        nodes = np.flatnonzero(comp == c)                     # ascending node id: the local numbering
        local = {int(n): i for i, n in enumerate(nodes)}
        parent = list(range(len(nodes)))
        count = [1] * len(nodes)

        def find(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x

        for e in np.flatnonzero(edge_comp == c):              # ascending edge index
            ra, rb = find(local[int(node[2 * e])]), find(local[int(node[2 * e + 1])])
            if ra == rb or count[ra] + count[rb] > max_track_length:
                continue
            ra, rb = min(ra, rb), max(ra, rb)
            parent[rb] = ra
            count[ra] += count[rb]
        for i, n in enumerate(nodes):
            label[n] = nodes[find(i)]
    return label


@pytest.mark.parametrize("cap", model.RANDOM_CAPS)
@pytest.mark.parametrize("seed", [model.RANDOM_SEED, 1, 2])
def test_reference_loop_equals_components_then_replay(seed, cap):
    ev, ef = model.random_graph(seed)
    node, _, _, root, _ = model.reference_sets(ev, ef, cap)
    assert np.array_equal(model.labels_of(root), components_then_replay(node, root.shape[0], cap))


def test_the_random_inputs_contain_every_case():
    """What the GPU tests' random graphs (model.random_graph(model.RANDOM_SEED) at caps 2, 5 and 50) exercise."""
    ev, ef = model.random_graph(model.RANDOM_SEED)
    assert len(set(ev.tolist())) >= 35 and 2000 <= ev.shape[0] // 2 <= 5000
    edges = np.stack([ev[0::2], ef[0::2], ev[1::2], ef[1::2]], axis=1)
    flipped = edges[:, [2, 3, 0, 1]]
    assert len(np.unique(edges, axis=0)) < len(edges), "no duplicate edge"
    lookup = set(map(tuple, edges.tolist()))
    assert any(tuple(f) in lookup for f in flipped.tolist()), "no edge in both orientations"
    seen = {}
    for cap in model.RANDOM_CAPS:
        r = model.build_tracks(ev, ef, 2, cap)
        assert 2000 <= r["num_nodes"] <= 5000
        seen[cap] = dict(oversize=r["num_oversize_components"], refused=r["refused"],
                         full=int(np.count_nonzero(r["set_sizes"] == cap)), small=r["num_small_tracks"],
                         inconsistent=r["num_inconsistent_features"])
        print(cap, seen[cap])
        assert r["num_oversize_components"] >= 3
        assert r["refused"] >= 1
        assert seen[cap]["full"] >= 1
    assert seen[2]["small"] >= 1 and seen[5]["small"] >= 1
    assert seen[5]["inconsistent"] >= 1 and seen[50]["inconsistent"] >= 1
