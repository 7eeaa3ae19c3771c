"""tmi_ba_match_features_cascade without a device: argument validation and the ABI mirrors, the device tests' inputs
checked for hash bits and distance decisions that are too close to call, the key formulation of the shortlist (step 4
of the ABI comment) against the model's restatement of the reference's loop, and the all-zero secondary projection
against the exact matcher's model."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cascade_matching_model as cm  # noqa: E402
import matching_model as mm  # noqa: E402
from theiasfm_amd import abi, lib, synth  # noqa: E402

CASES = cm.gpu_cases()
NO_RATIO = dict(use_lowes_ratio=False, keep_only_symmetric_matches=False, min_num_feature_matches=0)


def test_abi_structs_defaults_and_exports():
    # feature_matcher_options.h:45-71: symmetric, ratio test at 0.8, 30 matches
    assert C.sizeof(abi.CCascadeMatchOptions) == 24 and C.sizeof(abi.CCascadeMatchSummary) == 56
    o = abi.cascade_match_options()
    assert (o.use_lowes_ratio, o.keep_only_symmetric_matches, o.min_num_feature_matches, o.device,
            o.pairs_per_chunk) == (1, 1, 30, -1, 0)
    assert o.lowes_ratio == np.float32(0.8)
    L = lib.load()
    c = abi.CCascadeMatchOptions()
    L.tmi_ba_cascade_match_options_init(C.byref(c))
    assert bytes(c) == bytes(o) == bytes(abi.match_options())
    assert "tmi_ba_match_features_cascade" in lib.EXPORTS and "tmi_ba_cascade_match_options_init" in lib.EXPORTS
    assert hasattr(L, "tmi_ba_match_features_cascade")
    with pytest.raises(AttributeError):
        abi.cascade_match_options(no_such_field=1)


def test_argument_errors_come_before_the_device_and_no_device_after():
    begin, desc, _ = synth.make_matching_batch(2, 5, 8, seed=1)
    proj = synth.cascade_projections(8, 1)

    def status(*args, **kw):
        with pytest.raises(lib.EngineError) as e:
            lib.match_features_cascade(*args, **kw)
        return e.value.status

    assert status(begin, desc, proj, [0], [2]) == abi.ERR_INVALID_ARGUMENT
    bad = begin.copy()
    bad[1] = 11
    assert status(bad, desc, proj, [0], [1]) == abi.ERR_INVALID_ARGUMENT
    assert status(begin, desc, proj, [0], [1],
                  options=abi.cascade_match_options(min_num_feature_matches=-1)) == abi.ERR_INVALID_ARGUMENT
    assert status(begin, desc, proj, [0], [1],
                  options=abi.cascade_match_options(pairs_per_chunk=-1)) == abi.ERR_INVALID_ARGUMENT
    assert status(begin, np.zeros((10, 0), np.float32), np.zeros((188, 0), np.float32), [0],
                  [1]) == abi.ERR_INVALID_ARGUMENT
    # a null projections, straight through the library
    L = lib.load()
    o, ms = abi.cascade_match_options(), abi.CCascadeMatchSummary()
    p = np.zeros(1, np.int32)
    q = np.ones(1, np.int32)
    out8, out32, out64 = np.zeros(1, np.int8), np.zeros(1, np.int32), np.zeros(2, np.int64)
    st = L.tmi_ba_match_features_cascade(C.byref(o), 2, begin.ctypes.data, desc.ctypes.data, 8, None, 1, p.ctypes.data,
                                         q.ctypes.data, 0, out8.ctypes.data, out32.ctypes.data, out64.ctypes.data, None,
                                         None, None, None, None, C.byref(ms))
    assert st == abi.ERR_INVALID_ARGUMENT and b"projections" in L.tmi_ba_last_error()
    if L.tmi_ba_device_count() == 0:
        assert status(begin, desc, proj, [0], [1]) == abi.ERR_NO_DEVICE


def test_projection_generator_order_and_shape():
    p = synth.cascade_projections(5, 3)
    assert p.shape == (188, 5) and p.dtype == np.float32
    assert np.array_equal(p.ravel()[:7], synth._mt19937_normals(3, 7).astype(np.float32))  # row-major draw order
    assert np.array_equal(p, synth.cascade_projections(5, 3)) and not np.array_equal(p, synth.cascade_projections(5, 4))
    # std::mt19937(20140623) through a fresh std::normal_distribution<double>(0, 1) per draw, cast to float (libstdc++)
    want = [0.0034646887797862291, -0.11990603804588318, -0.29295551776885986, -0.36690011620521545]
    assert synth.cascade_projections(4).ravel()[:4].tolist() == [float(np.float32(v)) for v in want]
    z = synth.cascade_projections(5, 3, zero_secondary=True)
    assert np.array_equal(z[:128], p[:128]) and not z[128:].any()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_hash_bits_have_a_margin_or_are_flagged(case):
    """Each hash bit's relative margin |sum P t| / sum |P t| in float64 is >= BIT_MARGIN or the bit is flagged; the
    flagged bits are at most 0.5 % of the case's bits, and every bit that is not flagged equals the float64 bit."""
    b = case["image_begin"]
    bits = flagged = 0
    for m in range(len(b) - 1):
        x = case["descriptors"][b[m]:b[m + 1]]
        if x.shape[0] == 0:
            continue
        margin, bit64 = cm.bit_margins(x, case["projections"])
        bit32 = cm.project(x, case["projections"]) > 0
        alone = x.shape[0] == 1  # t == 0 exactly in every arithmetic: every bit is 0
        clear = (margin >= cm.BIT_MARGIN) & (not alone)
        assert np.array_equal(bit32[clear], bit64[clear])
        if alone:
            assert not bit32.any()
            continue
        bits += margin.size
        flagged += int(np.count_nonzero(~clear))
    print(case["name"], "bits", bits, "flagged", flagged)
    assert flagged <= 0.005 * bits


def _key_shortlist(code_i, ids_i, code2, ids2):
    """Step 4 as the ABI comment states it: among the unique candidates the 11 smallest under (Hamming distance,
    first shared group, column)."""
    shared = ids2 == ids_i[None, :]  # [N2, 6]
    total = int(shared.sum())
    if total <= 10:
        return total, []
    cols = np.nonzero(shared.any(axis=1))[0]
    first = shared[cols].argmax(axis=1)
    ham = (code2[cols] != code_i[None, :]).sum(axis=1)
    order = sorted(zip(ham.tolist(), first.tolist(), cols.tolist()))
    return total, [c for _, _, c in order[:11]]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_key_formulation_equals_the_reference_loop_and_decisions_have_a_margin(case):
    want = cm.model(case, min_num_feature_matches=0)
    b = case["image_begin"]
    imgs = [case["descriptors"][b[m]:b[m + 1]] for m in range(len(b) - 1)]
    hashes = [cm.hash_image(x, case["projections"]) for x in imgs]
    rows = dups = eleventh_ties = 0
    for (r, c), d in want["directions"].items():
        for i in range(imgs[r].shape[0] if imgs[c].shape[0] else 0):
            total, cols = _key_shortlist(hashes[r][0][i], hashes[r][1][i], hashes[c][0], hashes[c][1])
            assert total == d["totals"][i] and cols == d["lists"][i], (case["name"], r, c, i)
            if not cols:
                continue
            rows += 1
            shared = hashes[c][1] == hashes[r][1][i][None, :]
            dups += int((shared.sum(axis=1) > 1).sum())
            ham = np.sort((hashes[c][0][shared.any(axis=1)] != hashes[r][0][i][None, :]).sum(axis=1))
            eleventh_ties += int(ham.shape[0] > 11 and ham[10] == ham[11])
            assert len(cols) >= 2  # total > 10 and a column counts at most six times
            best, gap_best, gap_ratio, passes = cm.decision_margins(imgs[r][i], imgs[c], cols, 0.8)
            # the model decides as float64 does, with a margin (an image against itself: d0 == 0 exactly)
            assert gap_best >= cm.MARGIN and gap_ratio >= cm.MARGIN, (case["name"], r, c, i, gap_best, gap_ratio)
            assert best == d["best_i"][i] and passes == d["passed"][i]
    print(case["name"], "rows", rows, "duplicate candidates", dups, "ties at the eleventh place", eleventh_ties)
    assert rows > 0
    if case["name"].startswith("pooled"):
        assert dups > 100 and eleventh_ties > 0


def test_zero_secondary_projection_is_the_exact_matcher():
    """With an all-zero secondary projection and 2 <= N2 <= 11 every column is a candidate and shortlisted: the
    cascade model's (best, second, distance) equals matching_model.nearest_two on every row."""
    case = cm.zero_secondary_case()
    want = cm.model(case, **NO_RATIO)
    b = case["image_begin"]
    assert not want["image_bucket_ids"].any() and want["rows_skipped"] == 0
    for (r, c), d in want["directions"].items():
        a, cols = case["descriptors"][b[r]:b[r + 1]], case["descriptors"][b[c]:b[c + 1]]
        assert 2 <= cols.shape[0] <= 11
        bd, bi, sd = mm.nearest_two(mm.distances(a, cols))
        assert np.array_equal(bi, d["best_i"])
        assert bd.tobytes() == d["best_d"].tobytes() and sd.tobytes() == d["second_d"].tobytes()
        assert all(sorted(l) == list(range(cols.shape[0])) for l in d["lists"])
    exact = mm.match_batch(case["image_begin"], case["descriptors"], case["pair_image1"], case["pair_image2"], **NO_RATIO)
    for k in ("pair_status", "pair_num_forward", "pair_match_begin", "feature1", "feature2", "distance"):
        assert exact[k].tobytes() == want[k].tobytes(), k


def test_intended_branches_are_reached():
    d16 = cm.model(cm.pooled_case("pooled-d16"), min_num_feature_matches=0)
    totals = np.concatenate([d["totals"] for d in d16["directions"].values()])
    assert np.any(totals == 10) and np.any(totals == 11)
    for case in CASES[:4]:
        w = cm.model(case, min_num_feature_matches=0)
        assert w["rows_skipped"] > 0 and w["distance_evaluations"] > 0
    seen = set()
    for ratio in (True, False):
        seen.update(cm.model(cm.pooled_case("pooled-d16"), use_lowes_ratio=ratio)["pair_status"].tolist())
    assert seen == {0, 1}
    ids = cm.model(cm.long_bucket_case(), min_num_feature_matches=0)["image_bucket_ids"][40:]
    assert max(np.bincount(ids[:, g], minlength=1024).max() for g in range(6)) > 64


def test_ratio_is_squared_in_double_and_a_tie_is_kept():
    """sq is the double product of the float ratio, not 8.9's fp32 product; the row is dropped on `>`, so twelve
    identical rows against twelve identical columns (d0 == d1 == 0) are all kept, to column 0, where 8.9's strict `<`
    drops every one of them."""
    assert float(np.float32(0.8)) ** 2 != mm.ratio_sq(0.8)
    x = np.zeros((24, 4), np.float32)
    begin = np.asarray([0, 12, 24], np.int64)
    o = dict(keep_only_symmetric_matches=False, min_num_feature_matches=0)
    r = cm.match_batch(begin, x, synth.cascade_projections(4, 1), [0], [1], **o)
    assert r["feature1"].tolist() == list(range(12)) and not r["feature2"].any() and r["rows_skipped"] == 0
    assert mm.match_batch(begin, x, [0], [1], **o)["feature1"].shape[0] == 0
