"""The shared case list of the linear position estimator's tests (test_position_linear_cpu.py, test_gpu_position_linear.py).

Scenes follow the reference's linear_position_estimator_test.cc: cameras at 10 x rand, rotations 0.2 x rand, focal 800 on
a 1000 x 1000 image, points at rand + (0, 0, 20), relative poses from the truth with `noise` degrees of rotation about a
random axis on the relative rotation and on the translation direction.  Every case is the smallest shape at which a
kernel can still go wrong; what each is for stands beside it."""
import functools

import numpy as np
from scipy.spatial.transform import Rotation

from theiasfm_amd import abi, synth

import position_linear_model as model

INTRINSICS = {
    abi.PINHOLE: [800.0, 1.0, 0.0, 500.0, 500.0, 0.0, 0.0],
    abi.PINHOLE_RADIAL_TANGENTIAL: [800.0, 1.0, 0.0, 500.0, 500.0, 0.01, 0.001, 0.0, 0.001, -0.001],
    abi.FISHEYE: [800.0, 1.0, 0.0, 500.0, 500.0, 0.01, 0.001, 0.0, 0.0],
    abi.FOV: [800.0, 1.0, 500.0, 500.0, 0.1],
    abi.DIVISION_UNDISTORTION: [800.0, 1.0, 500.0, 500.0, -1e-8],
}


def _noise_rotation(rng, degrees):
    axis = rng.uniform(-1.0, 1.0, 3)
    return Rotation.from_rotvec(np.deg2rad(degrees) * axis / np.linalg.norm(axis)).as_matrix()


def scene(seed, num_views, pairs, num_tracks=50, noise=0.0, visible=None, camera_model=abi.PINHOLE, positions=None):
    """(Problem, ViewPairBatch, true positions [V, 3]).  visible(track) -> the views that observe it (default: all)."""
    rng = np.random.default_rng(seed)
    pos = 10.0 * rng.uniform(-1.0, 1.0, (num_views, 3)) if positions is None else np.asarray(positions, dtype=np.float64)
    rot = 0.2 * rng.uniform(-1.0, 1.0, (num_views, 3))
    points = np.concatenate([rng.uniform(-1.0, 1.0, (num_tracks, 3)) + [0.0, 0.0, 20.0], np.ones((num_tracks, 1))], axis=1)
    obs_view, obs_track = [], []
    for t in range(num_tracks):
        for v in (range(num_views) if visible is None else visible(t)):
            obs_view.append(v)
            obs_track.append(t)
    order = rng.permutation(len(obs_view))  # the call sorts: hand it an unsorted list
    obs_view, obs_track = np.array(obs_view, dtype=np.int32)[order], np.array(obs_track, dtype=np.int32)[order]
    K = INTRINSICS[camera_model]
    P = abi.Problem(np.concatenate([pos, rot], axis=1), np.zeros(num_views, dtype=np.int32),
                    np.zeros(num_views, dtype=np.uint8), [camera_model], [0, len(K)], K, np.ones(len(K), dtype=np.uint8),
                    points, np.zeros(num_tracks, dtype=np.uint8), obs_view, obs_track, np.zeros((len(obs_view), 2)))
    P.obs_xy[:] = synth.project(P)
    Rm = Rotation.from_rotvec(rot).as_matrix()
    rot2, pos2 = [], []
    for a, b in pairs:
        level = noise * rng.uniform(-1.0, 1.0, 2)
        rot2.append(Rotation.from_matrix(_noise_rotation(rng, level[0]) @ Rm[b] @ Rm[a].T).as_rotvec())
        d = pos[b] - pos[a]
        pos2.append(_noise_rotation(rng, level[1]) @ (Rm[a] @ (d / np.linalg.norm(d))))
    batch = abi.ViewPairBatch(rot, [a for a, _ in pairs], [b for _, b in pairs], np.array(rot2), np.array(pos2))
    return P, batch, pos


ALL4 = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
TRIANGLE = [(0, 1), (0, 2), (1, 2)]
DIAMOND = ((0, 1, 2), (0, 1, 3))  # two triplets that share the pair (0, 1)


def _triangles(*triplets):
    return sorted({p for a, b, c in triplets for p in ((a, b), (a, c), (b, c))})


def _wheel(rim):
    return sorted([(0, i) for i in range(1, rim + 1)] + [(i, i + 1) for i in range(1, rim)])


def _near(seed):
    """Views 4, 5, 6 within 0.01 of each other: every ray pair of their triplet is far below the angle threshold."""
    rng = np.random.default_rng(seed)
    pos = 10.0 * rng.uniform(-1.0, 1.0, (7, 3))
    pos[5] = pos[4] + [0.01, 0.0, 0.0]
    pos[6] = pos[4] + [0.0, 0.01, 0.0]
    return pos


# name -> (scene arguments, options).  Built lazily and once (case()).
_SPECS = {
    # order 6: the block as wide as the matrix.  One triplet alone leaves a double smallest eigenvalue (DEGENERATE): its
    # vector is compared through its eigen-residual, not through the gap bound
    "one_triplet": (dict(seed=1, num_views=3, pairs=TRIANGLE), {}),
    # the reference's two tests; the noise-free one is the singular case the shift exists for
    "four_clean": (dict(seed=2, num_views=4, pairs=ALL4), {}),
    "four_noisy": (dict(seed=3, num_views=4, pairs=ALL4, noise=1.0), {}),
    # a bow-tie: two pairs of triplets that share view 3 only -- two components of two, the tie goes to the smaller
    # number, and views 4, 5, 6 stay unestimated
    "bow_tie": (dict(seed=4, num_views=7, pairs=_triangles(*DIAMOND, (3, 4, 5), (3, 4, 6)), noise=0.5), {}),
    # components of 2 and 1 triplets, and an edge (6, 7) in no triplet
    "two_and_one": (dict(seed=5, num_views=8, pairs=_triangles((0, 1, 2), (0, 1, 3), (4, 5, 6)) + [(6, 7)], noise=0.5), {}),
    # views 3, 4, 5 share no track
    "no_common_track": (dict(seed=6, num_views=7, pairs=_triangles(*DIAMOND, (4, 5, 6)), noise=0.5,
                             visible=lambda t: (0, 1, 2, 3, 4 + t % 3)), {}),
    # every common track of (4, 5, 6) fails the angle test
    "angle_fails": (dict(seed=7, num_views=7, pairs=_triangles(*DIAMOND, (4, 5, 6)), noise=0.5, positions=_near(7)), {}),
    # (1, 2, 3) has no common track and is dropped in step 3: {(0,1,2), (1,2,3), (2,3,4)} falls apart and the two triplets
    # on views 5 .. 8 win -- the held view is view 5, not view 0
    "dropped_changes_choice": (dict(seed=8, num_views=9, noise=0.5,
                                    pairs=_triangles((0, 1, 2), (1, 2, 3), (2, 3, 4), (5, 6, 7), (6, 7, 8)),
                                    visible=lambda t: (0, 1, 2, 4, 5, 6, 7, 8) if t % 2 else (0, 2, 3, 4, 5, 6, 7, 8)), {}),
    # a hub in 80 triplets: more than a wavefront for the hub's rows.  A chain of triplets has a small eigen gap (9e-3
    # against |M|_inf = 516): the tolerance is tightened so that the comparison bound stays below 1e-6
    "wheel": (dict(seed=10, num_views=82, pairs=_wheel(81), num_tracks=8, noise=0.2), dict(tolerance=1e-12)),
}
# common-track counts around the wavefront and the in-LDS selection cap: even and odd median indices, both paths
for _n in (1, 2, 63, 64, 65, model.SELECT_CAP, model.SELECT_CAP + 1):
    _SPECS[f"tracks_{_n}"] = (dict(seed=20 + _n, num_views=4, pairs=ALL4, num_tracks=_n, noise=0.5), {})
for _m, _name in ((abi.PINHOLE_RADIAL_TANGENTIAL, "radtan"), (abi.FISHEYE, "fisheye"), (abi.FOV, "fov"),
                  (abi.DIVISION_UNDISTORTION, "division")):
    _SPECS[f"model_{_name}"] = (dict(seed=40 + _m, num_views=4, pairs=ALL4, noise=0.5, camera_model=_m), {})
# the vote: seeds found on the CPU (test_position_linear_cpu.py checks that both outcomes occur)
_SPECS["vote_a"] = (dict(seed=60, num_views=4, pairs=ALL4, noise=0.5), {})
_SPECS["vote_b"] = (dict(seed=61, num_views=4, pairs=ALL4, noise=0.5), {})

NAMES = list(_SPECS)
DEGENERATE = ("one_triplet",)


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(name, P, batch, truth, options, prep): the scene and the model's steps 1 to 5 on it, computed once."""
    spec, options = _SPECS[name]
    P, batch, truth = scene(**spec)
    prep = model.prepare(P, batch, options)
    # no ray pair within 1e-9 (relative) of the angle threshold: no inclusion decision can flip
    assert prep["angle_margin"] > 1e-9, (name, prep["angle_margin"])
    return dict(name=name, P=P, batch=batch, truth=truth, options=options, prep=prep)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The model's answer and the plain answer of a case, computed once and left unchanged."""
    c = case(name)
    return model.estimate(c["P"], c["batch"], c["options"], prep=c["prep"]), \
        (model.plain(c["P"], c["batch"], c["options"], prep=c["prep"]) if c["prep"]["M"] is not None else None)
