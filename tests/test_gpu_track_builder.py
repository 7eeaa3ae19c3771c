"""tmi_ba_build_tracks on the device against tests/track_builder_model.py (the reference's loop), by equality on every
output: track_begin, obs_view, obs_feature, endpoint_node, endpoint_label and the summary counts.  All integers, so no
tolerance anywhere.  The shapes are the smallest at which the kernels can go wrong: parent chains longer than a
wavefront and a workgroup (the shuffled path), every link contending for one root (the star), several oversize
components with refused merges (the random graphs, whose contents tests/test_track_builder_cpu.py asserts)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_builder_model as model  # noqa: E402
from theiasfm_amd import abi, lib  # noqa: E402

pytestmark = pytest.mark.gpu

ARRAYS = ("track_begin", "obs_view", "obs_feature", "endpoint_node", "endpoint_label")
COUNTS = ("num_nodes", "num_components", "num_oversize_components", "num_replayed_edges", "num_sets", "num_tracks",
          "num_observations", "num_small_tracks", "num_inconsistent_features")


def check(ev, ef, min_len=2, max_len=50):
    want = model.build_tracks(ev, ef, min_len, max_len)
    got = lib.build_tracks(ev, ef, abi.track_build_options(min_track_length=min_len, max_track_length=max_len),
                           want_nodes=True)
    assert got["status"] == 0
    for k in COUNTS:
        assert getattr(got["summary"], k) == want[k], k
    for k in ARRAYS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    return want, got


def path_graph(n, seed):
    """A path over n nodes, node i in view i % 7 (neighbours differ), its edges shuffled and randomly oriented."""
    rng = np.random.default_rng(seed)
    order = rng.permutation(n - 1)
    flip = rng.random(n - 1) < 0.5
    a = np.where(flip, order + 1, order)
    b = np.where(flip, order, order + 1)
    nodes = np.stack([a, b], axis=1).reshape(-1)
    return (nodes % 7).astype(np.uint32), (nodes // 7).astype(np.uint32)


@pytest.mark.parametrize("case", model.reference_cases(), ids=lambda c: c[0])
def test_reference_cases(case):
    _, ev, ef, min_len, max_len, expected = case
    want, _ = check(ev, ef, min_len, max_len)
    assert want["num_tracks"] == expected


def test_no_edge_and_one_edge():
    empty = np.zeros(0, dtype=np.uint32)
    got = lib.build_tracks(empty, empty, want_nodes=True)
    assert got["status"] == 0 and got["track_begin"].tolist() == [0] and got["obs_view"].shape == (0,)
    assert got["summary"].num_tracks == 0 and got["summary"].num_nodes == 0
    want, _ = check(np.array([3, 9], dtype=np.uint32), np.array([5, 5], dtype=np.uint32))
    assert want["num_tracks"] == 1 and want["obs_view"].tolist() == [3, 9]


def test_shuffled_path_longer_than_a_workgroup():
    ev, ef = path_graph(200, 5)
    want, _ = check(ev, ef, 2, 250)
    assert want["num_components"] == 1 and want["num_oversize_components"] == 0 and want["num_tracks"] == 1
    check(*path_graph(700, 6), 2, 1000)


def test_star_every_link_contends_for_one_root():
    leaves = np.arange(300)
    ev = np.stack([np.zeros(300, dtype=np.int64), 1 + leaves % 5], axis=1).reshape(-1).astype(np.uint32)
    ef = np.stack([np.zeros(300, dtype=np.int64), leaves // 5], axis=1).reshape(-1).astype(np.uint32)
    want, _ = check(ev, ef, 2, 400)
    assert want["num_nodes"] == 301 and want["num_tracks"] == 1 and want["num_inconsistent_features"] == 295
    check(ev, ef, 2, 50)  # the same star as one oversize component


@pytest.mark.parametrize("cap", model.RANDOM_CAPS)
def test_random_graph(cap):
    want, _ = check(*model.random_graph(model.RANDOM_SEED), 2, cap)
    assert want["num_oversize_components"] >= 3 and want["refused"] >= 1


def test_max_track_length_one_and_min_track_length_three():
    ev, ef = model.random_graph(3, num_tracks=60, num_edges=300)
    want, _ = check(ev, ef, 2, 1)
    assert want["num_tracks"] == 0 and want["num_small_tracks"] == want["num_nodes"]
    want, _ = check(ev, ef, 3, 50)
    assert want["num_small_tracks"] >= 1
    check(ev, ef, 1, 50)  # a set of one node is dropped whatever min_track_length says
    check(ev, ef, 1, 2)


def test_view_ids_up_to_the_last_and_shared_feature_indices():
    views = np.array([0, 1, 0x7fffffff, 0x80000000, 0xfffffffe, 0xffffffff], dtype=np.uint64)
    rng = np.random.default_rng(11)
    ev, ef = [], []
    while len(ev) < 400:
        a, b = rng.choice(6, size=2, replace=False)
        f = int(rng.integers(0, 8))  # the same feature index in both views: two different features
        ev += [views[a], views[b]]
        ef += [f, f if rng.random() < 0.8 else int(rng.integers(0, 8))]
    want, _ = check(np.array(ev, dtype=np.uint32), np.array(ef, dtype=np.uint32), 2, 4)
    assert want["obs_view"].max() == 0xffffffff and want["num_nodes"] <= 48


def test_capacity_protocol_and_repeatability():
    ev, ef = model.random_graph(model.RANDOM_SEED)
    o = abi.track_build_options(max_track_length=5)
    full = lib.build_tracks(ev, ef, o, want_nodes=True)
    nt, no = int(full["summary"].num_tracks), int(full["summary"].num_observations)
    for tcap, ocap in ((nt - 1, no), (nt, no - 1), (0, 0)):
        small = lib.build_tracks(ev, ef, o, track_capacity=tcap, obs_capacity=ocap)
        assert small["status"] == abi.ERR_CAPACITY
        assert (small["summary"].num_tracks, small["summary"].num_observations) == (nt, no)
    sized = lib.build_tracks(ev, ef, o, track_capacity=nt, obs_capacity=no, want_nodes=True)
    assert sized["status"] == 0
    for k in ARRAYS:  # the same input twice: the same bytes
        assert sized[k].tobytes() == full[k].tobytes(), k


def test_invalid_arguments_leave_the_outputs_untouched():
    L = lib.load()
    ev = np.array([0, 1, 1, 2], dtype=np.uint32)
    ef = np.zeros(4, dtype=np.uint32)
    same_view = np.array([0, 1, 2, 2], dtype=np.uint32)

    def call(options=True, summary=True, E=2, view=ev, feature=ef, tcap=4, ocap=8, no_begin=False, no_obs=False, **o):
        begin = np.full(5, -7, dtype=np.int64)
        obs = [np.full(8, 77, dtype=np.uint32) for _ in range(2)]
        ends = [np.full(4, 77, dtype=np.uint32) for _ in range(2)]
        opts, ts = abi.track_build_options(**o), abi.CTrackBuildSummary()
        st = L.tmi_ba_build_tracks(C.byref(opts) if options else None, E, view.ctypes.data if view is not None else None,
                                   feature.ctypes.data if feature is not None else None, tcap, ocap,
                                   None if no_begin else begin.ctypes.data, None if no_obs else obs[0].ctypes.data,
                                   None if no_obs else obs[1].ctypes.data, ends[0].ctypes.data, ends[1].ctypes.data,
                                   C.byref(ts) if summary else None)
        assert (begin == -7).all() and all((a == 77).all() for a in obs + ends)
        return st

    for kwargs in (dict(options=False), dict(summary=False), dict(view=None), dict(feature=None), dict(no_begin=True),
                   dict(no_obs=True), dict(E=-1), dict(tcap=-1), dict(ocap=-1), dict(E=1 << 30),
                   dict(max_track_length=0), dict(min_track_length=0), dict(view=same_view)):
        assert call(**kwargs) == abi.ERR_INVALID_ARGUMENT, kwargs
