"""tmi_ba_match_features on the device against the numpy fp32 model (tests/matching_model.py): every comparison is
EQUALITY -- the statuses, the forward counts, the offsets, both index arrays and the distances as uint32 bit patterns.
Nothing is left out and no tolerance is used; tests/test_matching_cpu.py shows that the inputs hold no decision that is
too close to call other than the planted exact ties."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matching_model as mm  # noqa: E402
from theiasfm_amd import abi, lib  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("pair_status", "pair_num_forward", "pair_match_begin", "feature1", "feature2", "distance")
COMBOS = [(r, s) for r in (True, False) for s in (True, False)]


def run(case, pairs_per_chunk=0, match_capacity=None, **options):
    o = dict(mm.DEFAULTS)
    o.update(options)
    return lib.match_features(*mm.case_args(case), options=abi.match_options(
        use_lowes_ratio=int(o["use_lowes_ratio"]), lowes_ratio=o["lowes_ratio"],
        keep_only_symmetric_matches=int(o["keep_only_symmetric_matches"]),
        min_num_feature_matches=o["min_num_feature_matches"], device=0, pairs_per_chunk=pairs_per_chunk),
        match_capacity=match_capacity)


def assert_equal(got, want, what):
    assert got["status"] == 0, what
    for k in KEYS:
        g, w = got[k], want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.shape, w.shape)
        if k == "distance":
            g, w = g.view(np.uint32), w.view(np.uint32)
        assert np.array_equal(g, w), (what, k, np.nonzero(g != w)[0][:8])


def check(case, **options):
    got = run(case, **options)
    want = mm.model(case, **options)
    assert_equal(got, want, (case["name"], options))
    return got, want


@pytest.mark.parametrize("dim", mm.DIMS)
def test_sizes_and_dimensions(dim):
    """N1, N2 from {0, 1, 2, 3, 63, 64, 65, 129, 257} crossed sparsely, at every dimension; the option combination
    rotates with the dimension (all four run in test_four_option_combinations)."""
    ratio, sym = COMBOS[mm.DIMS.index(dim) % 4]
    got, want = check(mm.size_case(dim), use_lowes_ratio=ratio, keep_only_symmetric_matches=sym,
                      min_num_feature_matches=2)
    assert set(want["pair_status"].tolist()) == {0, 1}  # both outcomes occur
    assert got["summary"].num_matches == want["feature1"].shape[0] > 0


@pytest.mark.parametrize("ratio,sym", COMBOS)
def test_four_option_combinations(ratio, sym):
    check(mm.size_case(33), use_lowes_ratio=ratio, keep_only_symmetric_matches=sym, min_num_feature_matches=0)


def test_large_pair():
    got, want = check(mm.large_case())
    assert want["pair_status"].tolist() == [0] and want["feature1"].shape[0] > 1000
    assert got["summary"].distance_evaluations == 2 * 2000 * 1500


def test_min_num_feature_matches_hit_and_missed_by_one():
    case = mm.count_case()
    off = dict(use_lowes_ratio=False)  # (with the ratio test this input's forward matches are all symmetric)
    base = mm.model(case, min_num_feature_matches=0, **off)
    F, S = int(base["pair_num_forward"][0]), int(base["feature1"].shape[0])
    assert 0 < S < F
    one_way = dict(keep_only_symmetric_matches=False, **off)
    assert check(case, min_num_feature_matches=F, **one_way)[0]["pair_status"].tolist() == [0]      # forward: hit
    assert check(case, min_num_feature_matches=F + 1, **one_way)[0]["pair_status"].tolist() == [1]  # missed by one
    assert check(case, min_num_feature_matches=S, **off)[0]["pair_status"].tolist() == [0]          # symmetric: hit
    got, _ = check(case, min_num_feature_matches=S + 1, **off)                                      # missed by one,
    assert got["pair_status"].tolist() == [1] and got["pair_num_forward"].tolist() == [F]           # forward passed
    assert got["feature1"].shape[0] == 0


def test_shared_image_self_pair_and_transpose():
    case = mm.size_case(128)
    got, _ = check(case, min_num_feature_matches=0)
    pairs = list(zip(case["pair_image1"].tolist(), case["pair_image2"].tolist()))
    b = got["pair_match_begin"]
    assert sum(8 in p for p in pairs) >= 6 and (8, 8) in pairs
    sl = lambda p: slice(b[p], b[p + 1])  # noqa: E731
    for p, (i, j) in enumerate(pairs):
        if i == j or (j, i) not in pairs:
            continue
        q = pairs.index((j, i))
        fwd = sorted(zip(got["feature1"][sl(p)].tolist(), got["feature2"][sl(p)].tolist(),
                         got["distance"][sl(p)].view(np.uint32).tolist()))
        rev = sorted(zip(got["feature2"][sl(q)].tolist(), got["feature1"][sl(q)].tolist(),
                         got["distance"][sl(q)].view(np.uint32).tolist()))
        assert fwd == rev, (i, j)
    # an image against itself: every row matches a row at distance 0 (itself, or its lower-indexed duplicate)
    p = pairs.index((8, 8))
    assert np.all(got["distance"][sl(p)] == 0) and np.all(got["feature2"][sl(p)] <= got["feature1"][sl(p)])


def test_planted_duplicates():
    case = mm.integer_case()
    assert case["meta"]["duplicate_rows"]
    b = case["image_begin"]
    on, _ = check(case, keep_only_symmetric_matches=False, min_num_feature_matches=0)
    off, _ = check(case, use_lowes_ratio=False, keep_only_symmetric_matches=False, min_num_feature_matches=0)
    pairs = list(zip(case["pair_image1"].tolist(), case["pair_image2"].tolist()))
    seen = 0
    for m, dst, src in case["meta"]["duplicate_rows"]:
        for p, (i, j) in enumerate(pairs):
            if j != m:
                continue
            lo = slice(off["pair_match_begin"][p], off["pair_match_begin"][p + 1])
            f2 = off["feature2"][lo]
            hit = np.nonzero((f2 == dst) | (f2 == src))[0]
            # best equals second: with the ratio off the lower index wins, with it on strict < rejects the row
            assert np.all(f2[hit] == min(dst, src))
            rows = off["feature1"][lo][hit]
            kept = on["feature1"][on["pair_match_begin"][p]:on["pair_match_begin"][p + 1]]
            assert not np.intersect1d(rows, kept).size
            seen += hit.size
    assert seen > 0
    assert b[-1] == case["descriptors"].shape[0]


def test_equal_best_distances_across_and_within_column_tiles():
    case = mm.tile_tie_case()
    on, _ = check(case, keep_only_symmetric_matches=False, min_num_feature_matches=0)
    off, _ = check(case, use_lowes_ratio=False, keep_only_symmetric_matches=False, min_num_feature_matches=0)
    n = off["pair_match_begin"][1]
    assert off["feature1"][:n].tolist() == [0, 1, 2, 3] and off["feature2"][:n].tolist() == [5, 70, 63, 3]
    assert np.all(off["distance"][:n] == np.float32(2.0 ** -12))
    assert on["pair_num_forward"][0] == 0  # every query's best equals its second


def test_integer_and_zero_descriptors():
    for combo in COMBOS:
        check(mm.integer_case(), use_lowes_ratio=combo[0], keep_only_symmetric_matches=combo[1],
              min_num_feature_matches=3)
    got, _ = check(mm.zero_case(), use_lowes_ratio=False, min_num_feature_matches=0)
    # all distances 0: every row picks column 0, and only row 0 is column 0's pick
    assert got["feature1"].tolist() == [0, 0, 0] and got["feature2"].tolist() == [0, 0, 0]
    assert check(mm.zero_case(), min_num_feature_matches=0)[0]["feature1"].shape[0] == 0


def test_subnormal_squares_are_kept():
    case = mm.subnormal_case()
    got, want = check(case, use_lowes_ratio=False, min_num_feature_matches=0)
    d = got["distance"]
    tiny = np.finfo(np.float32).tiny
    assert np.float32(np.abs(case["descriptors"]).max()) ** 2 < tiny  # every square is subnormal (or 0)
    assert d.shape[0] > 10 and np.count_nonzero(d) == d.shape[0] and np.all(d < 64 * tiny)
    assert len(set(got["feature2"].tolist())) > 10  # (flushed, every row would pick column 0)
    check(case, min_num_feature_matches=0)


def test_chunking_and_repeat_give_identical_bytes():
    case = mm.size_case(32)
    outs = [run(case, pairs_per_chunk=c, min_num_feature_matches=2) for c in (1, 3, 0, 0)]
    assert [o["summary"].num_chunks for o in outs[:3]] == [len(mm.SIZE_PAIRS), (len(mm.SIZE_PAIRS) + 2) // 3, 1]
    for o in outs[1:]:
        for k in KEYS:
            assert o[k].tobytes() == outs[0][k].tobytes(), k
    assert_equal(outs[0], mm.model(case, min_num_feature_matches=2), "chunked")


def test_capacity_one_too_small():
    case = mm.size_case(32)
    want = mm.model(case, min_num_feature_matches=2)
    total = int(want["pair_match_begin"][-1])
    got = run(case, match_capacity=total - 1, min_num_feature_matches=2)
    assert got["status"] == abi.ERR_CAPACITY and got["summary"].num_matches == total
    for k in ("pair_status", "pair_num_forward", "pair_match_begin"):
        assert np.array_equal(got[k], want[k]), k
    assert_equal(run(case, match_capacity=total, min_num_feature_matches=2), want, "exact capacity")
