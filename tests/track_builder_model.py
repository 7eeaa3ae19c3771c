"""A model of tmi_ba_build_tracks written from the REFERENCE'S LOOP, not from the device's decomposition:
TrackBuilder::AddFeatureCorrespondence (track_builder.cc:62-77) with its global FindOrInsert (:133-151),
ConnectedComponents::AddEdge on every edge in order with the cap (connected_components.h:87-108: union by size, the
tie attaching root2 to root1), Extract (:111-119) and BuildTracks (track_builder.cc:79-131).  The ordering rules of
steps 4 to 6 of the ABI comment (labels, the always-dropped singleton, lowest node id per view, ascending output) are
applied to that result.  Also here: the inputs the CPU and the GPU tests share."""
import numpy as np


def reference_sets(endpoint_view, endpoint_feature, max_track_length):
    """FindOrInsert ids and the reference's capped union-find over the edges in order.  Returns (endpoint_node [2E],
    node_view, node_feature, root [num_nodes], refused): root[n] is the id of the root of n's set as the reference's
    loop leaves it, refused the number of merges the cap refused."""
    ev = np.asarray(endpoint_view, dtype=np.uint64)
    ef = np.asarray(endpoint_feature, dtype=np.uint64)
    assert ev.shape == ef.shape and ev.ndim == 1 and ev.shape[0] % 2 == 0
    features = {}          # (view, feature) -> id, num_features_ the next one
    node_view, node_feature = [], []
    endpoint_node = np.zeros(ev.shape[0], dtype=np.int64)
    for i in range(ev.shape[0]):
        key = (int(ev[i]), int(ef[i]))
        if key not in features:
            features[key] = len(features)
            node_view.append(key[0])
            node_feature.append(key[1])
        endpoint_node[i] = features[key]
    n = len(features)
    root_id = list(range(n))   # disjoint_set_[node].id
    root_size = [1] * n        # disjoint_set_[node].size

    def find_root(node):
        path = []
        while root_id[node] != node:
            path.append(node)
            node = root_id[node]
        for p in path:         # `*parent = *root` on the way back
            root_id[p] = node
        return node

    refused = 0
    for e in range(ev.shape[0] // 2):
        assert ev[2 * e] != ev[2 * e + 1], "CHECK_NE(view_id1, view_id2)"
        r1 = find_root(int(endpoint_node[2 * e]))
        r2 = find_root(int(endpoint_node[2 * e + 1]))
        if r1 == r2:
            continue
        if root_size[r1] + root_size[r2] > max_track_length:
            refused += 1
            continue
        if root_size[r1] < root_size[r2]:
            root_size[r2] += root_size[r1]
            root_id[r1] = r2
        else:
            root_size[r1] += root_size[r2]
            root_id[r2] = r1
    root = np.array([find_root(i) for i in range(n)], dtype=np.int64)
    return (endpoint_node, np.array(node_view, dtype=np.uint32), np.array(node_feature, dtype=np.uint32), root, refused)


def labels_of(root):
    """The smallest node id of every node's set (step 4's label), from any array that is constant on a set."""
    root = np.asarray(root, dtype=np.int64)
    smallest = np.full(root.shape[0], root.shape[0], dtype=np.int64)
    np.minimum.at(smallest, root, np.arange(root.shape[0]))
    return smallest[root]


def tracks_from_labels(label, node_view, node_feature, endpoint_node, min_track_length):
    """Steps 4 to 6 on a labelling, and the summary counts that follow from it."""
    label = np.asarray(label, dtype=np.int64)
    n = label.shape[0]
    size = np.bincount(label, minlength=n) if n else np.zeros(0, dtype=np.int64)
    sets = np.flatnonzero(size > 0)                      # ascending label
    emitted = size >= max(int(min_track_length), 2)      # a set of one node is always dropped
    track_begin, obs_view, obs_feature = [0], [], []
    inconsistent = 0
    members = {int(s): [] for s in sets}
    for node in range(n):                                # ascending node id inside a set
        members[int(label[node])].append(node)
    for s in sets:
        if not emitted[s]:
            continue
        seen = set()
        for node in members[int(s)]:
            v = int(node_view[node])
            if v in seen:
                inconsistent += 1
                continue
            seen.add(v)
            obs_view.append(v)
            obs_feature.append(int(node_feature[node]))
        track_begin.append(len(obs_view))
    num_tracks = len(track_begin) - 1
    return dict(track_begin=np.array(track_begin, dtype=np.int64), obs_view=np.array(obs_view, dtype=np.uint32),
                obs_feature=np.array(obs_feature, dtype=np.uint32),
                endpoint_node=np.asarray(endpoint_node).astype(np.uint32),
                endpoint_label=label[np.asarray(endpoint_node, dtype=np.int64)].astype(np.uint32),
                num_nodes=n, num_sets=int(sets.shape[0]), num_tracks=num_tracks, num_observations=len(obs_view),
                num_small_tracks=int(sets.shape[0]) - num_tracks, num_inconsistent_features=inconsistent,
                set_sizes=size[sets])


def unconstrained_components(endpoint_node, num_nodes):
    """The label (smallest node id) of every node's component with no cap, by propagating minima in numpy."""
    a = np.asarray(endpoint_node, dtype=np.int64)[0::2]
    b = np.asarray(endpoint_node, dtype=np.int64)[1::2]
    label = np.arange(num_nodes, dtype=np.int64)
    while True:
        m = np.minimum(label[a], label[b])
        nxt = label.copy()
        np.minimum.at(nxt, a, m)
        np.minimum.at(nxt, b, m)
        nxt = nxt[nxt]                                   # pointer jumping
        if np.array_equal(nxt, label):
            return label
        label = nxt


def build_tracks(endpoint_view, endpoint_feature, min_track_length=2, max_track_length=50):
    """The whole call: what tmi_ba_build_tracks must return, plus `refused` and the graph counts of the summary."""
    ev = np.asarray(endpoint_view)
    node, nview, nfeat, root, refused = reference_sets(ev, endpoint_feature, max_track_length)
    out = tracks_from_labels(labels_of(root), nview, nfeat, node, min_track_length)
    comp = unconstrained_components(node, out["num_nodes"])
    csize = np.bincount(comp, minlength=out["num_nodes"]) if out["num_nodes"] else np.zeros(0, dtype=np.int64)
    over = csize > max_track_length
    out.update(refused=refused, num_components=int(np.count_nonzero(csize)),
               num_oversize_components=int(np.count_nonzero(over)),
               num_replayed_edges=int(np.count_nonzero(over[comp[node[0::2]]])) if ev.shape[0] else 0)
    return out


# ---- the inputs the tests share ---------------------------------------------------------------------
def reference_cases():
    """The reference's five tests (track_builder_test.cc:64-199) as (name, endpoint_view, endpoint_feature, min, max,
    tracks expected).  Feature(i, i) of a view becomes that view's local index in order of first use, as the shim maps
    it."""
    def edges(corr):
        local = {}
        ev, ef = [], []
        for (v1, f1, v2, f2) in corr:
            for v, f in ((v1, f1), (v2, f2)):
                ids = local.setdefault(v, {})
                ev.append(v)
                ef.append(ids.setdefault(f, len(ids)))
        return np.array(ev, dtype=np.uint32), np.array(ef, dtype=np.uint32)

    pairs = [(0, 1), (0, 1), (1, 2), (1, 2)]
    chain = [(i, 0, i + 1, 0) for i in range(5)]
    return [
        ("ConsistentTracks",) + edges([(a, i, b, i) for i, (a, b) in enumerate(pairs)]) + (2, 10, 4),
        ("SingletonTracks",) + edges([(0, 0, 1, 0), (1, 0, 2, 0)]) + (2, 2, 1),
        ("InconsistentTracks",) + edges([(a, 0, b, i + 1) for i, (a, b) in enumerate(pairs)]) + (2, 10, 2),
        ("MaxTrackLength",) + edges(chain) + (2, 2, 3),
        ("MinTrackLength",) + edges(chain + [(0, 1, 1, 1)]) + (3, 10, 1),
    ]


def random_graph(seed, num_views=40, num_tracks=600, num_edges=3000, cross=0.2):
    """About num_views views, a few thousand nodes and edges: true tracks of 2 to 12 views, edges between two members
    of a track in both orientations, a fraction `cross` joining different tracks (oversize components, inconsistent
    features), and every tenth edge a duplicate of an earlier one."""
    rng = np.random.default_rng(seed)
    members = []
    next_feature = np.zeros(num_views, dtype=np.int64)
    for _ in range(num_tracks):
        views = rng.choice(num_views, size=int(rng.integers(2, 13)), replace=False)
        members.append([(int(v), int(next_feature[v])) for v in views])
        next_feature[views] += 1
    ev, ef = [], []
    while len(ev) < 2 * num_edges:
        if ev and rng.random() < 0.1:
            e = int(rng.integers(len(ev) // 2))
            a, b = (ev[2 * e], ef[2 * e]), (ev[2 * e + 1], ef[2 * e + 1])
        else:
            t = members[int(rng.integers(num_tracks))]
            i, j = rng.choice(len(t), size=2, replace=False)
            a = t[int(i)]
            b = t[int(j)]
            if rng.random() < cross:
                u = members[int(rng.integers(num_tracks))]
                b = u[int(rng.integers(len(u)))]
        if a[0] == b[0]:
            continue
        if rng.random() < 0.5:
            a, b = b, a
        ev += [a[0], b[0]]
        ef += [a[1], b[1]]
    return np.array(ev, dtype=np.uint32), np.array(ef, dtype=np.uint32)


RANDOM_SEED = 20261019
RANDOM_CAPS = (2, 5, 50)
