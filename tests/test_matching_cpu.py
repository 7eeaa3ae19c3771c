"""tmi_ba_match_features without a device: the reference's three tests (brute_force_feature_matcher_test.cc) restated
on the numpy model with their data recipes, the fp32 model against an independent float64 evaluation wherever a
decision is not too close to call, the device tests' inputs checked for such decisions, chunking, the ratio constant,
and the ABI mirrors."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matching_model as mm  # noqa: E402
from theiasfm_amd import abi, lib, synth  # noqa: E402

K = 10  # kNumDescriptors = kNumDescriptorDimensions = 10


def _normalized(v):
    v = np.asarray(v, dtype=np.float32)
    return (v / np.sqrt(np.sum(v * v, dtype=np.float32))).astype(np.float32)


def test_reference_no_options():
    # ten copies of the normalised constant vector in both images; everything off, min 0: EXPECT_GT(NumMatches, 0).
    # Every distance is 0, so every row keeps its best: ten matches, and by the tie rule all of them to column 0.
    a = np.tile(_normalized(np.ones(K)), (K, 1))
    r = mm.match_pair(a, a.copy(), use_lowes_ratio=False, keep_only_symmetric_matches=False, min_num_feature_matches=0)
    assert r["status"] == 0 and r["feature1"].tolist() == list(range(K)) and r["feature2"].tolist() == [0] * K
    assert np.all(r["distance"] == 0)


def test_reference_ratio_test():
    # The reference's test expects one image-pair entry (NumMatches counts PAIRS, and min is 0), not a surviving
    # match: the two candidates are nearly equidistant, the ratio test rejects the row and the pair has no match.
    a = _normalized(np.ones(K))[None, :]
    b0 = np.ones(K, np.float32)
    b0[0] = 0.9
    b1 = np.ones(K, np.float32)
    b1[0] = 0.89
    b = np.stack([_normalized(b0), _normalized(b1)])
    r = mm.match_pair(a, b, use_lowes_ratio=True, keep_only_symmetric_matches=False, min_num_feature_matches=0)
    assert r["status"] == 0 and r["num_forward"] == 0 and r["feature1"].shape[0] == 0
    off = mm.match_pair(a, b, use_lowes_ratio=False, keep_only_symmetric_matches=False, min_num_feature_matches=0)
    assert off["feature1"].tolist() == [0] and off["feature2"].tolist() == [0]


def _symmetric_inputs():
    a1 = np.zeros(K, np.float32)
    a1[0] = 1.0
    a = np.stack([_normalized(np.ones(K)), a1])
    b0 = np.ones(K, np.float32)
    b0[0] = 0
    b1 = np.ones(K, np.float32)
    b1[1] = b1[2] = 0
    return a, np.stack([_normalized(b0), _normalized(b1)])


def test_reference_symmetric_matches():
    # Both columns are nearer to row 0 than to row 1; row 0 prefers column 0, row 1 prefers column 1 and column 1
    # prefers row 0: one symmetric match, (0, 0).  (The reference's EXPECT_EQ(NumMatches, 1) counts the pair.)
    a, b = _symmetric_inputs()
    r = mm.match_pair(a, b, use_lowes_ratio=False, keep_only_symmetric_matches=True, min_num_feature_matches=0)
    assert r["status"] == 0 and r["num_forward"] == 2
    assert list(zip(r["feature1"].tolist(), r["feature2"].tolist())) == [(0, 0)]
    one_way = mm.match_pair(a, b, use_lowes_ratio=False, keep_only_symmetric_matches=False, min_num_feature_matches=0)
    assert list(zip(one_way["feature1"].tolist(), one_way["feature2"].tolist())) == [(0, 0), (1, 1)]


def test_ratio_sq_is_the_double_of_the_fp32_product():
    r = np.float32(0.8)
    assert mm.ratio_sq(0.8) == float(np.float32(r * r))
    assert mm.ratio_sq(0.8) != 0.8 * 0.8 and mm.ratio_sq(0.8) != float(r) * float(r)
    assert mm.ratio_sq(0.8).hex() == "0x1.47ae160000000p-1"


def test_distance_is_symmetric_and_ordered():
    rng = np.random.default_rng(0)
    a = rng.normal(size=(7, 13)).astype(np.float32)
    b = rng.normal(size=(5, 13)).astype(np.float32)
    d = mm.distances(a, b)
    assert d.dtype == np.float32 and np.array_equal(d.T, mm.distances(b, a))
    acc = np.float32(0)
    for k in range(13):
        t = np.float32(a[2, k] - b[3, k])
        acc = np.float32(acc + np.float32(t * t))
    assert acc == d[2, 3]


def _directions(case):
    b = case["image_begin"]
    for p, (i1, i2) in enumerate(zip(case["pair_image1"], case["pair_image2"])):
        for fwd in (True, False):
            r, c = (i1, i2) if fwd else (i2, i1)
            yield p, int(r), int(c), case["descriptors"][b[r]:b[r + 1]], case["descriptors"][b[c]:b[c + 1]]


@pytest.mark.parametrize("case", mm.gpu_cases(), ids=lambda c: c["name"])
def test_device_inputs_have_no_close_call_and_fp32_agrees_with_float64(case):
    """Every decision of the device tests' inputs is either planted (an exact tie: float64 agrees that the two
    distances are EQUAL, and the tie rule decides), exact (integer-valued data: fp32 and float64 compute the same
    numbers) or has a margin of at least MARGIN -- and wherever the margin is that large the fp32 model decides as
    float64 does."""
    planted = mm.planted_rows(case)
    seen = set()
    for p, r, c, a, b in _directions(case):
        if (r, c) in seen:
            continue
        seen.add((r, c))
        ref = mm.reference_decisions(a, b)
        bd, bi, sd = mm.nearest_two(mm.distances(a, b))
        ok32 = mm.ratio_pass(bd, bi, sd, b.shape[0], True, 0.8)
        for i in range(a.shape[0]):
            if b.shape[0] < 2:
                assert bi[i] == ref["best"][i]
                continue
            tie = ref["best_d"][i] == ref["second_d"][i]
            if tie:
                # the tie rule: the lower of the equal columns, in both models; strict < rejects the row
                assert case["exact"] or (r, i) in planted or (c, int(ref["best"][i])) in planted, (case["name"], r, c, i)
                assert bi[i] == ref["best"][i] and bd[i] == sd[i] and not ok32[i]
                continue
            if not case["exact"]:
                assert ref["gap_best"][i] >= mm.MARGIN, (case["name"], r, c, i, ref["gap_best"][i])
                assert ref["gap_ratio"][i] >= mm.MARGIN, (case["name"], r, c, i, ref["gap_ratio"][i])
            if ref["gap_best"][i] >= mm.MARGIN:
                assert bi[i] == ref["best"][i]
            if ref["gap_ratio"][i] >= mm.MARGIN and ref["gap_best"][i] >= mm.MARGIN:
                assert ok32[i] == ref["passes"][i]


def test_model_chunked_equals_whole():
    case = mm.size_case(33)
    whole = mm.match_batch(*mm.case_args(case), min_num_feature_matches=2)
    for step in (1, 3):
        part = mm.match_batch(*mm.case_args(case), pairs_per_chunk=step, min_num_feature_matches=2)
        for k in whole:
            assert whole[k].dtype == part[k].dtype and whole[k].tobytes() == part[k].tobytes(), k


def test_planted_duplicates_and_ties_follow_the_tie_rule():
    case = mm.integer_case()
    b = case["image_begin"]
    d = case["descriptors"]
    assert case["meta"]["tie_rows"] and case["meta"]["duplicate_rows"]
    for q, m, lo, hi in case["meta"]["tie_rows"]:
        dist = mm.distances(d[b[0] + q][None, :], d[b[m]:b[m + 1]])[0]
        assert dist[lo] == dist[hi] == 1.0 and dist.min() == 1.0


def test_abi_structs_and_defaults():
    assert C.sizeof(abi.CMatchOptions) == 24
    assert C.sizeof(abi.CMatchSummary) == 40
    o = abi.match_options()
    assert (o.use_lowes_ratio, o.keep_only_symmetric_matches, o.min_num_feature_matches, o.device,
            o.pairs_per_chunk) == (1, 1, 30, -1, 0)
    assert o.lowes_ratio == np.float32(0.8)
    L = lib.load()
    c = abi.CMatchOptions()
    L.tmi_ba_match_options_init(C.byref(c))
    assert bytes(c) == bytes(o)
    assert "tmi_ba_match_features" in lib.EXPORTS and abi.STATUS_NAMES[abi.ERR_CAPACITY] == "CAPACITY"
    with pytest.raises(AttributeError):
        abi.match_options(no_such_field=1)


def test_argument_errors_come_before_the_device():
    begin, desc, _ = synth.make_matching_batch(2, 5, 8, seed=1)
    with pytest.raises(lib.EngineError) as e:
        lib.match_features(begin, desc, [0], [2])
    assert e.value.status == abi.ERR_INVALID_ARGUMENT
    bad = begin.copy()
    bad[1] = 11
    with pytest.raises(lib.EngineError) as e:
        lib.match_features(bad, desc, [0], [1])
    assert e.value.status == abi.ERR_INVALID_ARGUMENT
    with pytest.raises(lib.EngineError) as e:
        lib.match_features(begin, desc, [0], [1], options=abi.match_options(min_num_feature_matches=-1))
    assert e.value.status == abi.ERR_INVALID_ARGUMENT
    with pytest.raises(lib.EngineError) as e:
        lib.match_features(begin, np.zeros((10, 0), np.float32), [0], [1])
    assert e.value.status == abi.ERR_INVALID_ARGUMENT
