"""tmi_ba_guided_epipolar_match on the device against the pure-Python model (tests/guided_matching_model.py) on the
cases of tests/guided_matching_cases.py: groups, candidate counts and added matches are equal, the distances in their
bytes.  tests/test_guided_matching_cpu.py shows that no decision of these inputs is too close to call."""
import numpy as np
import pytest

import guided_matching_cases as gc
from theiasfm_amd import abi, lib

pytestmark = pytest.mark.gpu

CASES = gc.cases()
IDS = [c["name"] for c in CASES]


def run(case, **kw):
    options = abi.guided_match_options(device=0, **kw.pop("options", {}))
    return lib.guided_epipolar_match(*gc.case_args(case), options=options, want_groups=True, **kw)


def assert_equal(out, ref):
    assert out["status"] == 0
    for k in ("pair_status", "pair_num_groups", "pair_added_begin", "feature_group", "group_num_candidates", "feature1",
              "feature2"):
        np.testing.assert_array_equal(out[k], ref[k], err_msg=k)
    assert out["distance"].tobytes() == ref["distance"].tobytes()
    np.testing.assert_array_equal(out["group_endpoints"], ref["group_endpoints"])


@pytest.fixture(scope="module", params=CASES, ids=IDS)
def full(request):
    return request.param, run(request.param)


def test_device_equals_model(full):
    case, out = full
    ref = gc.model(case)
    assert_equal(out, ref)
    s = out["summary"]
    assert s.num_pairs == len(gc.PAIRS) and s.num_added == len(ref["feature1"])
    assert s.num_groups == int(ref["pair_num_groups"].sum())
    assert s.num_candidates == int(ref["group_num_candidates"].sum())
    assert s.distance_evaluations == sum(len(f) * len(c) for r in ref["pairs"]
                                         for f, c in zip(r["group_features"], r["group_candidates"]))
    assert list(out["pair_status"]) == [0, 0, 0, 0, 1, 0, 0] and s.num_pairs_ok == 6
    assert s.kernel_seconds > 0 and s.seconds >= s.kernel_seconds


def test_two_runs_give_the_same_bytes(full):
    case, out = full
    again = run(case)
    for k in ("pair_status", "pair_num_groups", "pair_added_begin", "feature_group", "group_num_candidates",
              "group_endpoints", "feature1", "feature2", "distance"):
        assert out[k].tobytes() == again[k].tobytes(), k


def test_other_options_equal_the_model():
    case = CASES[0]
    o = gc.OTHER_OPTIONS
    assert_equal(run(case, options=dict(o)), gc.model(case, **o))


def test_masked_batch_equals_the_rows_of_the_full_one(full):
    case, out = full
    mask = np.array([1, 0, 1, 0, 0, 1, 1], np.uint8)
    part = run(case, pair_mask=mask)
    P = len(mask)
    assert part["summary"].num_pairs == int(mask.sum())
    for p in range(P):
        a = slice(part["pair_added_begin"][p], part["pair_added_begin"][p + 1])
        rows = slice(out["pair_row"][p], out["pair_row"][p + 1])
        if not mask[p]:
            assert part["pair_status"][p] == -1 and a.stop == a.start and part["pair_num_groups"][p] == 0
            assert (part["feature_group"][rows] == -1).all() and (part["group_num_candidates"][rows] == 0).all()
            continue
        b = slice(out["pair_added_begin"][p], out["pair_added_begin"][p + 1])
        assert part["pair_status"][p] == out["pair_status"][p]
        for k in ("feature1", "feature2", "distance"):
            assert part[k][a].tobytes() == out[k][b].tobytes(), (p, k)
        for k in ("feature_group", "group_num_candidates", "group_endpoints"):
            assert part[k][rows].tobytes() == out[k][rows].tobytes(), (p, k)


def test_a_pair_alone_with_its_stream_equals_its_rows(full):
    case, out = full
    p = 6  # the sparse pair: every group draws from the stream
    a = gc.case_args(case)
    m = slice(a[6][p], a[6][p + 1])
    alone = lib.guided_epipolar_match(a[0], a[1], a[2], a[3][p:p + 1], a[4][p:p + 1], a[5][p:p + 1],
                                      [0, m.stop - m.start], a[7][m], a[8][m], pair_stream=[p],
                                      options=abi.guided_match_options(device=0), want_groups=True)
    b = slice(out["pair_added_begin"][p], out["pair_added_begin"][p + 1])
    for k in ("feature1", "feature2", "distance"):
        assert alone[k].tobytes() == out[k][b].tobytes(), k
    rows = slice(out["pair_row"][p], out["pair_row"][p + 1])
    assert alone["group_num_candidates"].tobytes() == out["group_num_candidates"][rows].tobytes()


def test_empty_batch_is_ok():
    case = CASES[0]
    a = gc.case_args(case)
    out = lib.guided_epipolar_match(a[0], a[1], a[2], [], [], np.zeros((0, 9)), [0], [], [],
                                    options=abi.guided_match_options(device=0))
    assert out["status"] == 0 and out["summary"].num_added == 0 and out["pair_added_begin"].tolist() == [0]
    masked = run(case, pair_mask=np.zeros(len(gc.PAIRS), np.uint8))
    assert masked["status"] == 0 and (masked["pair_status"] == -1).all() and masked["summary"].rows_uploaded == 0


def test_capacity_overflow_is_reported_and_nothing_is_written(full):
    case, out = full
    total = int(out["pair_added_begin"][-1])
    assert total > 3
    small = run(case, added_capacity=total - 1)
    assert small["status"] == abi.ERR_CAPACITY and small["summary"].num_added == total
    np.testing.assert_array_equal(small["pair_added_begin"], out["pair_added_begin"])
    np.testing.assert_array_equal(small["pair_status"], out["pair_status"])
    for arr in small["added_arrays"]:
        assert arr.shape == (total - 1,) and not arr.any()
    exact = run(case, added_capacity=total)
    assert exact["status"] == 0 and exact["distance"].tobytes() == out["distance"].tobytes()


def test_both_directions_upload_each_image_once():
    case = CASES[0]
    a = gc.case_args(case)
    n = int(a[0][1])
    F = np.stack([a[5][3], a[5][3].reshape(3, 3).T.reshape(9)])
    out = lib.guided_epipolar_match(a[0], a[1], a[2], [0, 1], [1, 0], F, [0, 0, 0], [], [],
                                    options=abi.guided_match_options(device=0))
    assert out["status"] == 0 and out["summary"].rows_uploaded == 2 * n and out["summary"].num_pairs == 2


def test_guided_result_adds_no_input_match(full):
    case, out = full
    a = gc.case_args(case)
    p = 0
    given = set(zip(a[7][a[6][p]:a[6][p + 1]].tolist(), a[8][a[6][p]:a[6][p + 1]].tolist()))
    b = slice(out["pair_added_begin"][p], out["pair_added_begin"][p + 1])
    added = set(zip(out["feature1"][b].tolist(), out["feature2"][b].tolist()))
    assert added and not (added & given)
    assert not (set(out["feature1"][b].tolist()) & {f for f, _ in given})
