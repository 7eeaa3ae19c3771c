"""-m "not gpu": the numpy model of the linear position estimator (tests/position_linear_model.py) against brute force and
against the reference's own tests, the comparison bound of the GPU test, and every refusal of
tmi_ba_estimate_global_positions_linear through the C ABI (argument errors come before the device is looked for)."""
import ctypes as C

import numpy as np
import pytest

import position_linear_cases as cases
import position_linear_model as model
from theiasfm_amd import abi, lib

BOUND_C = 4.0  # test_gpu_position_linear.py holds the device to this multiple


# ---- step 1: the graphs of the reference's triplet_extractor_test.cc ---------------------------------------------------
GRAPHS = {
    "one_triplet": [(0, 1), (0, 2), (1, 2)],
    "two_sharing_an_edge": [(0, 1), (0, 2), (1, 2), (1, 3), (2, 3)],
    "two_sharing_a_view": [(0, 1), (0, 2), (1, 2), (2, 3), (2, 4), (3, 4)],
    "two_disjoint": [(0, 1), (0, 2), (1, 2), (3, 4), (3, 5), (4, 5)],
    "no_triplet": [(0, 1), (1, 2), (2, 3), (0, 3)],
    "complete_5": [(a, b) for a in range(5) for b in range(a + 1, 5)],
    "wheel_70": [(0, i) for i in range(1, 71)] + [(i, i + 1) for i in range(1, 70)],
}


@pytest.mark.parametrize("name", list(GRAPHS))
def test_triplets_against_brute_force(name):
    pairs = GRAPHS[name]
    rng = np.random.default_rng(len(pairs))
    pairs = [pairs[i] for i in rng.permutation(len(pairs))]  # the batch order is the caller's
    V = max(b for _, b in pairs) + 1
    v1, v2 = [a for a, _ in pairs], [b for _, b in pairs]
    views, index = model.find_triplets(V, v1, v2)
    brute = model.brute_force_triplets(V, v1, v2)
    assert [tuple(t) for t in views.tolist()] == brute
    for (a, b, c), (e_ab, e_ac, e_bc) in zip(brute, index.tolist()):
        assert (pairs[e_ab], pairs[e_ac], pairs[e_bc]) == ((a, b), (a, c), (b, c))


# ---- step 4 ----------------------------------------------------------------------------------------------------------------
def _components(triplets, alive=None):
    pairs = sorted({p for a, b, c in triplets for p in ((a, b), (a, c), (b, c))})
    index = {p: e for e, p in enumerate(pairs)}
    tp = [(index[(a, b)], index[(a, c)], index[(b, c)]) for a, b, c in triplets]
    return model.components(tp, [True] * len(triplets) if alive is None else alive)


def test_component_rule():
    # a shared PAIR joins, a shared view does not
    label, chosen = _components([(0, 1, 2), (0, 1, 3), (3, 4, 5)])
    assert label.tolist() == [0, 0, 2] and chosen == 0
    label, chosen = _components([(0, 1, 2), (2, 3, 4)])
    assert label.tolist() == [0, 1] and chosen == 0  # a tie: the smallest triplet number
    # the larger component wins although it comes later
    label, chosen = _components([(0, 1, 2), (3, 4, 5), (3, 4, 6)])
    assert label.tolist() == [0, 1, 1] and chosen == 1
    # a dropped triplet neither joins nor counts
    label, chosen = _components([(0, 1, 2), (1, 2, 3), (2, 3, 4), (5, 6, 7), (6, 7, 8)], [True, False, True, True, True])
    assert label.tolist() == [0, -1, 2, 3, 3] and chosen == 3
    assert _components([(0, 1, 2)], [False])[1] == -1


def test_dropped_triplet_changes_the_choice():
    p = cases.case("dropped_changes_choice")["prep"]
    assert p["triplet_num_used"].tolist()[1] == 0 and p["chosen"].tolist() == [3, 4]
    assert p["views"][0] == 5  # the held view is not view 0
    with_all, _ = model.components(p["triplet_pair"], [True] * 5)
    assert (with_all == 0).sum() == 3  # had (1, 2, 3) survived, the first three would have won


# ---- step 3: the scenes of compute_triplet_baseline_ratios_test.cc -------------------------------------------------------
@pytest.mark.parametrize("noise", [0.0, 1.0])
def test_baselines_recover_the_ratios(noise):
    """Three views, perfect relative poses of unit baseline: the baseline is (1, |c0 c2| / |c0 c1|, |c1 c2| / |c0 c1|)
    (their test's 1e-8 without noise; with pixel noise its 0.05 relative)."""
    P, batch, pos = cases.scene(71, 3, cases.TRIANGLE, num_tracks=100)
    if noise:
        P.obs_xy += np.random.default_rng(5).normal(0.0, noise, P.obs_xy.shape)
    views, pairs = model.find_triplets(3, batch.pair_view1, batch.pair_view2)
    base, common, used, dropped, _ = model.baselines(P, batch, views, pairs, 2.0)
    d01, d02, d12 = (np.linalg.norm(pos[b] - pos[a]) for a, b in ((0, 1), (0, 2), (1, 2)))
    assert common[0] == 100 and used[0] + dropped <= 100 and used[0] > 50
    np.testing.assert_allclose(base[0], [1.0, d02 / d01, d12 / d01], rtol=0.05 if noise else 1e-8)


# ---- the reference's two estimator tests -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tolerance", [("four_clean", 1e-4), ("four_noisy", 0.25)])
def test_reference_estimator_tests(name, tolerance):
    c = cases.case(name)
    est, plain = cases.reference(name)
    assert est["usable"] and est["converged"] and est["estimated"].all()
    for result in (est, plain):
        assert model.umeyama_errors(result["positions"], c["truth"]).max() < tolerance


def test_both_vote_outcomes_occur():
    flipped = set()
    for seed in range(60, 72):
        P, batch, _ = cases.scene(seed, 4, cases.ALL4, noise=0.5)
        out = model.estimate(P, batch)
        assert abs(out["sign_votes"]) == 6  # a clean geometry: every edge agrees
        flipped.add(out["flipped"])
    assert flipped == {0, 1}
    assert {cases.reference("vote_a")[0]["flipped"], cases.reference("vote_b")[0]["flipped"]} == {0, 1}


# ---- the comparison bound -------------------------------------------------------------------------------------------------
def test_comparison_bound():
    """|model - plain| against derived_bound(1, ...) over the case list: the largest ratio measured is 0.115
    (model_fisheye); the GPU test takes c = 4, about 35 x that.  No case of the list has a bound above 1e-6 at c = 4,
    the one degenerate case (a double smallest eigenvalue) apart, which the GPU test holds to its eigen-residual."""
    worst = 0.0
    for name in cases.NAMES:
        est, plain = cases.reference(name)
        assert est["usable"] and est["converged"], name
        w = plain["eigenvalues"]
        if name in cases.DEGENERATE:
            assert w[1] - w[0] < 1e-6 * est["matrix_norm"]
            continue
        unit = model.derived_bound(1.0, est["order"], est["options"]["tolerance"], est["matrix_norm"], w[1] - w[0])
        ratio = np.linalg.norm(est["positions"] - plain["positions"]) / unit
        print(name, "ratio", ratio, "bound at c", BOUND_C * unit)
        assert BOUND_C * unit <= 1e-6, name
        worst = max(worst, ratio)
    assert worst <= BOUND_C / 8.0


# ---- refusals --------------------------------------------------------------------------------------------------------------
def _call(P, batch, options=None, capacity=0, null=()):
    """The raw C call with sentinel outputs; returns (status, outputs untouched?)."""
    L = lib.load()
    V = batch.num_views
    pos, est = np.full((V, 3), 3.5), np.full(V, 7, dtype=np.uint8)
    o = options if options is not None else abi.linear_position_options()
    cp, cb, ps = P.as_c(), batch.as_c(), abi.CLinearPositionSummary()
    args = dict(problem=C.byref(cp), batch=C.byref(cb), options=C.byref(o), position=pos.ctypes.data,
                estimated=est.ctypes.data, summary=C.byref(ps))
    args.update({name: None for name in null})
    st = L.tmi_ba_estimate_global_positions_linear(args["problem"], args["batch"], args["options"], -1, args["position"],
                                                   args["estimated"], capacity, None, None, None, None, None, None,
                                                   args["summary"])
    return st, bool((pos == 3.5).all() and (est == 7).all())


def _batch(c, **changes):
    b = c["batch"].copy()
    for k, v in changes.items():
        setattr(b, k, v)
    return b


def test_refusals():
    c = cases.case("four_noisy")
    P, good = c["P"], c["batch"]
    assert hasattr(lib.load(), "tmi_ba_estimate_global_positions_linear")
    bad = []
    for name in ("problem", "batch", "options", "position", "estimated", "summary"):
        bad.append(("null " + name, P, good, None, (name,)))
    empty = abi.ViewPairBatch(good.view_rotation, [], [], np.zeros((0, 3)), np.zeros((0, 3)))
    bad.append(("no pair", P, empty, None, ()))
    b = good.copy()
    b.pair_view2 = b.pair_view2.copy()
    b.pair_view2[0] = 4
    bad.append(("view out of range", P, b, None, ()))
    b = good.copy()
    b.pair_view1, b.pair_view2 = b.pair_view2.copy(), b.pair_view1.copy()
    bad.append(("view1 >= view2", P, b, None, ()))
    b = good.copy()
    b.pair_view1[1], b.pair_view2[1] = b.pair_view1[0], b.pair_view2[0]
    bad.append(("repeated pair", P, b, None, ()))
    for field in ("pair_rotation2", "pair_position2", "view_rotation"):
        b = good.copy()
        getattr(b, field)[1, 2] = np.nan
        bad.append(("non-finite " + field, P, b, None, ()))
    for kw in (dict(max_iterations=0), dict(tolerance=0.0), dict(tolerance=np.inf), dict(relative_shift=-1e-9),
               dict(relative_shift=np.nan), dict(min_triangulation_angle_degrees=0.0),
               dict(min_triangulation_angle_degrees=180.0)):
        bad.append((str(kw), P, good, abi.linear_position_options(**kw), ()))
    Q = P.copy()
    Q.obs_camera[0] = 4
    bad.append(("observation index", Q, good, None, ()))
    Q = P.copy()
    Q.obs_camera[1], Q.obs_point[1] = Q.obs_camera[0], Q.obs_point[0]
    bad.append(("track observed twice", Q, good, None, ()))
    five = abi.ViewPairBatch(np.zeros((5, 3)), good.pair_view1, good.pair_view2, good.pair_rotation2, good.pair_position2)
    bad.append(("num_cameras != num_views", P, five, None, ()))
    for why, problem, batch, options, null in bad:
        st, untouched = _call(problem, batch, options, null=null)
        assert st == abi.ERR_INVALID_ARGUMENT, why
        assert untouched, why
    assert _call(P, good, capacity=-1)[0] == abi.ERR_INVALID_ARGUMENT
    # a view without an edge may have any orientation
    P6, b6, _ = cases.scene(3, 5, cases.ALL4, noise=1.0)
    b6.view_rotation[4] = np.nan
    assert _call(P6, b6)[0] != abi.ERR_INVALID_ARGUMENT


def test_options_init():
    o = abi.CLinearPositionOptions()
    lib.load().tmi_ba_linear_position_options_init(C.byref(o))
    d = abi.linear_position_options()
    for name, _ in abi.CLinearPositionOptions._fields_:
        assert getattr(o, name) == getattr(d, name), name
    assert (o.max_iterations, o.tolerance, o.relative_shift, o.seed, o.min_triangulation_angle_degrees) == \
        (1000, 1e-10, 1e-9, 0, 2.0)
