"""tmi_ba_match_features_cascade on the device against the numpy fp32 model (tests/cascade_matching_model.py), which
is written from the reference's loop: every comparison is EQUALITY -- the statuses, the forward counts, the offsets,
both index arrays, the distances as uint32 bit patterns, image_hash, image_bucket_ids, rows_skipped,
candidates_examined and the number of exact distances.  tests/test_cascade_matching_cpu.py shows that the inputs hold
no distance decision under the margin and bounds the share of hash bits that are close to call."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cascade_matching_model as cm  # noqa: E402
from theiasfm_amd import abi, lib  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("pair_status", "pair_num_forward", "pair_match_begin", "feature1", "feature2", "distance")
HASH_KEYS = ("image_hash", "image_bucket_ids")
COUNTERS = ("rows_skipped", "candidates_examined", "distance_evaluations")


def run(case, pairs_per_chunk=0, match_capacity=None, **options):
    o = dict(cm.DEFAULTS)
    o.update(options)
    return lib.match_features_cascade(*cm.case_args(case), options=abi.cascade_match_options(
        use_lowes_ratio=int(o["use_lowes_ratio"]), lowes_ratio=o["lowes_ratio"],
        keep_only_symmetric_matches=int(o["keep_only_symmetric_matches"]),
        min_num_feature_matches=o["min_num_feature_matches"], device=0, pairs_per_chunk=pairs_per_chunk),
        match_capacity=match_capacity, want_hash=True)


def assert_equal(got, want, what, keys=KEYS + HASH_KEYS):
    assert got["status"] == 0, what
    for k in keys:
        g, w = got[k], want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.shape, w.shape)
        if k == "distance":
            g, w = g.view(np.uint32), w.view(np.uint32)
        assert np.array_equal(g, w), (what, k, np.argwhere(g != w)[:8].tolist())
    for k in COUNTERS:
        assert getattr(got["summary"], k) == want[k], (what, k, getattr(got["summary"], k), want[k])


def check(case, **options):
    got = run(case, **options)
    want = cm.model(case, **options)
    assert_equal(got, want, (case["name"], options))
    return got, want


@pytest.mark.parametrize("name", list(cm.POOLED))
def test_pooled_inputs(name):
    got, want = check(cm.pooled_case(name), min_num_feature_matches=0)
    assert want["rows_skipped"] > 0 and want["feature1"].shape[0] > 0  # rows skipped and rows matched
    assert got["summary"].num_matches == want["feature1"].shape[0]
    totals = np.concatenate([d["totals"] for d in want["directions"].values()])
    if name == "pooled-d16":
        assert np.any(totals == 10) and np.any(totals == 11)  # the candidate-count rule on both sides of its bound


def test_bucket_longer_than_a_wavefront():
    case = cm.long_bucket_case()
    got, want = check(case, use_lowes_ratio=False, keep_only_symmetric_matches=False, min_num_feature_matches=0)
    counts = np.stack([np.bincount(want["image_bucket_ids"][40:, g], minlength=1024) for g in range(6)])
    assert counts.max() > 64
    assert max(int(d["totals"].max()) for d in want["directions"].values()) > 2 * 53  # more than two strides
    assert want["feature1"].shape[0] > 0
    check(case, min_num_feature_matches=0)


def test_images_of_0_1_2_rows_and_self_pairs():
    case = cm.tiny_case()
    got, want = check(case, use_lowes_ratio=False, min_num_feature_matches=0)
    pairs = list(zip(case["pair_image1"].tolist(), case["pair_image2"].tolist()))
    b = got["pair_match_begin"]
    p = pairs.index((3, 3))
    assert b[p + 1] - b[p] > 0 and np.all(got["distance"][b[p]:b[p + 1]] == 0)  # an image against itself
    for q, (i, j) in enumerate(pairs):
        if 0 in (i, j):
            assert b[q + 1] == b[q] and got["pair_num_forward"][q] == 0  # an empty image has no matches
    check(case, min_num_feature_matches=1)


def test_zero_secondary_projection_is_the_exact_matcher():
    """Every column is a candidate and shortlisted (N2 <= 11), so the cascade call equals tmi_ba_match_features on the
    device: no ratio test (the two calls type it differently), one direction, no minimum."""
    case = cm.zero_secondary_case()
    o = dict(use_lowes_ratio=False, keep_only_symmetric_matches=False, min_num_feature_matches=0)
    got, want = check(case, **o)
    exact = lib.match_features(case["image_begin"], case["descriptors"], case["pair_image1"], case["pair_image2"],
                               options=abi.match_options(use_lowes_ratio=0, keep_only_symmetric_matches=0,
                                                         min_num_feature_matches=0, device=0))
    assert np.all(np.diff(case["image_begin"])[case["pair_image2"]] <= 11)
    for k in KEYS:
        assert got[k].tobytes() == exact[k].tobytes(), k
    assert got["summary"].rows_skipped == 0 and np.all(got["image_bucket_ids"] == 0)
    assert got["summary"].distance_evaluations == exact["summary"].distance_evaluations


def test_chunking_and_repeat_give_identical_bytes():
    case = cm.tiny_case()
    outs = [run(case, pairs_per_chunk=c, use_lowes_ratio=False, min_num_feature_matches=0) for c in (1, 3, 0, 0)]
    P = case["pair_image1"].shape[0]
    assert [o["summary"].num_chunks for o in outs[:3]] == [P, (P + 2) // 3, 1]
    for o in outs[1:]:
        for k in KEYS + HASH_KEYS:
            assert o[k].tobytes() == outs[0][k].tobytes(), k
        for k in COUNTERS:
            assert getattr(o["summary"], k) == getattr(outs[0]["summary"], k), k
    assert_equal(outs[0], cm.model(case, use_lowes_ratio=False, min_num_feature_matches=0), "chunked")


@pytest.mark.parametrize("ratio", (True, False))
@pytest.mark.parametrize("sym", (True, False))
@pytest.mark.parametrize("min_matches", (0, 30))
def test_options_grid(ratio, sym, min_matches):
    check(cm.pooled_case("pooled-d16"), use_lowes_ratio=ratio, keep_only_symmetric_matches=sym,
          min_num_feature_matches=min_matches)


def test_capacity_one_too_small():
    case = cm.pooled_case("pooled-d32")
    o = dict(use_lowes_ratio=False, min_num_feature_matches=0)
    want = cm.model(case, **o)
    total = int(want["pair_match_begin"][-1])
    assert total > 1
    got = run(case, match_capacity=total - 1, **o)
    assert got["status"] == abi.ERR_CAPACITY and got["summary"].num_matches == total
    for k in ("pair_status", "pair_num_forward", "pair_match_begin") + HASH_KEYS:
        assert np.array_equal(got[k], want[k]), k
    assert_equal(run(case, match_capacity=total, **o), want, "exact capacity")
