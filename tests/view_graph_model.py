"""CPU model of the two view-graph calls (tmi_ba_largest_connected_component and
tmi_ba_orientations_from_maximum_spanning_tree), numpy and plain Python only, written independently of the device
code: components by breadth-first search, the spanning tree by Kruskal with Python's sorted() on the reference's key
(math/graph/minimum_spanning_tree.h:83), rooting by a stack, and Ceres' AngleAxisToRotationMatrix /
RotationMatrixToAngleAxis restated with their small-angle and near-pi branches."""
import math
from types import SimpleNamespace

import numpy as np

EPS = np.finfo(np.float64).eps


# ---- Ceres' two conversions ------------------------------------------------------------------------------------------
def angle_axis_to_rotation_matrix(aa):
    """ceres::AngleAxisToRotationMatrix: Rodrigues' formula, first order below theta^2 = epsilon."""
    x, y, z = (float(a) for a in aa)
    theta2 = x * x + y * y + z * z
    if theta2 > EPS:
        theta = math.sqrt(theta2)
        wx, wy, wz = x / theta, y / theta, z / theta
        c, s = math.cos(theta), math.sin(theta)
        k = 1.0 - c
        return np.array([[c + wx * wx * k, wx * wy * k - wz * s, wy * s + wx * wz * k],
                         [wz * s + wx * wy * k, c + wy * wy * k, -wx * s + wy * wz * k],
                         [-wy * s + wx * wz * k, wx * s + wy * wz * k, c + wz * wz * k]])
    return np.array([[1.0, -z, y], [z, 1.0, -x], [-y, x, 1.0]])


def rotation_matrix_to_angle_axis(R):
    """ceres::RotationMatrixToAngleAxis of Ceres 1.x: RotationMatrixToQuaternion (on the trace, or on the largest
    diagonal entry when the trace is negative: the near-pi branch), then QuaternionToAngleAxis (atan2 on the negated
    pair for a negative scalar part; the factor 2 where the vector part vanishes: the small-angle branch)."""
    trace = R[0, 0] + R[1, 1] + R[2, 2]
    q = [0.0] * 4
    if trace >= 0.0:
        t = math.sqrt(trace + 1.0)
        q[0] = 0.5 * t
        t = 0.5 / t
        q[1] = (R[2, 1] - R[1, 2]) * t
        q[2] = (R[0, 2] - R[2, 0]) * t
        q[3] = (R[1, 0] - R[0, 1]) * t
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = math.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[i + 1] = 0.5 * t
        t = 0.5 / t
        q[0] = (R[k, j] - R[j, k]) * t
        q[j + 1] = (R[j, i] + R[i, j]) * t
        q[k + 1] = (R[k, i] + R[i, k]) * t
    s2 = q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
    k = 2.0
    if s2 > 0.0:
        s = math.sqrt(s2)
        c = q[0]
        two_theta = 2.0 * (math.atan2(-s, -c) if c < 0.0 else math.atan2(s, c))
        k = two_theta / s
    return np.array([q[1] * k, q[2] * k, q[3] * k])


def relative_rotation(o1, o2):
    """RelativeRotationFromOrientations of the reference's test: the angle-axis of R(o2) R(o1)^T."""
    return rotation_matrix_to_angle_axis(angle_axis_to_rotation_matrix(o2) @ angle_axis_to_rotation_matrix(o1).T)


def rotation_angle(R):
    """The angle of a rotation matrix in [0, pi], accurate near 0: atan2(|skew part| / 2, (trace - 1) / 2)."""
    s = 0.5 * math.sqrt((R[2, 1] - R[1, 2]) ** 2 + (R[0, 2] - R[2, 0]) ** 2 + (R[1, 0] - R[0, 1]) ** 2)
    return math.atan2(s, 0.5 * (R[0, 0] + R[1, 1] + R[2, 2] - 1.0))


def rotation_difference(a, b):
    """The angle of R(a) R(b)^T for two angle-axis vectors: how far apart they are AS ROTATIONS."""
    return rotation_angle(angle_axis_to_rotation_matrix(a) @ angle_axis_to_rotation_matrix(b).T)


def compute_orientation(parent_orientation, rotation2, parent_is_view1):
    """ComputeOrientation (orientations_from_maximum_spanning_tree.cc:62-84)."""
    Rp = angle_axis_to_rotation_matrix(parent_orientation)
    Rr = angle_axis_to_rotation_matrix(rotation2)
    return rotation_matrix_to_angle_axis((Rr if parent_is_view1 else Rr.T) @ Rp)


# ---- the graph ---------------------------------------------------------------------------------------------------------
def _alive(E, mask):
    return np.ones(E, dtype=bool) if mask is None else np.asarray(mask).astype(bool)


def components(V, v1, v2, mask=None):
    """tmi_ba_largest_connected_component.  label: the smallest view of the view's component (breadth-first search from
    the views in ascending order, so a component's first view is its smallest)."""
    E = len(v1)
    alive = _alive(E, mask)
    adj = [[] for _ in range(V)]
    for e in range(E):
        if alive[e]:
            adj[v1[e]].append(int(v2[e]))
            adj[v2[e]].append(int(v1[e]))
    label = np.full(V, -1, dtype=np.int32)
    sizes = {}
    for s in range(V):
        if label[s] >= 0:
            continue
        label[s] = s
        queue, head = [s], 0
        while head < len(queue):
            u = queue[head]
            head += 1
            for w in adj[u]:
                if label[w] < 0:
                    label[w] = s
                    queue.append(w)
        sizes[s] = len(queue)
    with_edges = {c: n for c, n in sizes.items() if n >= 2}
    largest = min(with_edges, key=lambda c: (-with_edges[c], c)) if with_edges else -1
    in_largest = (label == largest).astype(np.uint8)
    keep = np.array([alive[e] and label[v1[e]] == largest for e in range(E)], dtype=np.uint8).reshape(E)
    n_alive = int(alive.sum())
    return SimpleNamespace(
        label=label, in_largest=in_largest, keep=keep, num_components=len(with_edges), largest_label=int(largest),
        largest_num_views=with_edges.get(largest, 0), num_pairs_kept=int(keep.sum()),
        num_pairs_removed=n_alive - int(keep.sum()),
        num_views_removed=sum(with_edges.values()) - with_edges.get(largest, 0))


def kruskal(V, v1, v2, weight, keep):
    """The reference's Extract (minimum_spanning_tree.h:70-100) on the kept edges with weight -num_verified_matches:
    sorted() on (weight, (node1, node2)) with the pair ordered as a ViewIdPair (a repeated pair keeps its edge order,
    as a stable sort leaves it), then union-find."""
    order = sorted((e for e in range(len(v1)) if keep[e]),
                   key=lambda e: (-int(weight[e]), min(int(v1[e]), int(v2[e])), max(int(v1[e]), int(v2[e])), e))
    root = list(range(V))

    def find(x):
        while root[x] != x:
            root[x] = root[root[x]]
            x = root[x]
        return x

    in_tree = np.zeros(len(v1), dtype=np.uint8)
    for e in order:
        a, b = find(int(v1[e])), find(int(v2[e]))
        if a != b:
            root[a] = b
            in_tree[e] = 1
    return in_tree


def spanning_tree(V, v1, v2, weight, rotation2, mask=None, root_view=-1, orientation=None):
    """tmi_ba_orientations_from_maximum_spanning_tree.  root_view outside the largest component: ValueError."""
    cc = components(V, v1, v2, mask)
    out = SimpleNamespace(component=cc, usable=0, num_tree_pairs=0, tree_depth=0, root_view=-1,
                          orientation=np.full((V, 3), np.nan) if orientation is None else np.array(orientation, float),
                          parent=np.full(V, -1, np.int32), parent_pair=np.full(V, -1, np.int32),
                          depth=np.full(V, -1, np.int32), in_tree=np.zeros(len(v1), np.uint8))
    if cc.largest_label < 0:
        return out
    root = cc.largest_label if root_view < 0 else root_view
    if not cc.in_largest[root]:
        raise ValueError("root_view is outside the largest component")
    out.in_tree = kruskal(V, v1, v2, weight, cc.keep)
    adj = [[] for _ in range(V)]
    for e in np.flatnonzero(out.in_tree):
        adj[v1[e]].append((int(v2[e]), int(e), True))    # (neighbour, edge, this view is the edge's view1)
        adj[v2[e]].append((int(v1[e]), int(e), False))
    out.depth[root] = 0
    out.orientation[root] = 0.0
    stack = [root]
    while stack:
        u = stack.pop()
        for w, e, u_is_view1 in adj[u]:
            if out.depth[w] >= 0:
                continue
            out.depth[w] = out.depth[u] + 1
            out.parent[w] = u
            out.parent_pair[w] = e
            out.orientation[w] = compute_orientation(out.orientation[u], rotation2[e], u_is_view1)
            stack.append(w)
    out.usable = 1
    out.num_tree_pairs = int(out.in_tree.sum())
    out.tree_depth = int(out.depth.max())
    out.root_view = int(root)
    return out
