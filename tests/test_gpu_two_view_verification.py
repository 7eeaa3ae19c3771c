"""-m gpu: tmi_ba_verify_two_views (two_view_verify_kernels.h around two_view_lm_kernel) against its own stages, the CPU
model (tests/two_view_verification_model.py) and the oracle.

A status is a comparison of a computed number with a threshold, so the device and the model may disagree where that
number sits on the threshold: a correspondence may be SET ASIDE only when the model's margin for it (|dot - cos_min|,
|err^2 - max^2| / max^2) is below 1e-9, and at most 0.1 % of a test's correspondences may be.  The model itself, run on
the same batches in natural and in permuted order on the CPU (test_two_view_verification_cpu.py
::test_model_in_permuted_order_agrees_with_itself, and the seeds 51, 73 and 74 below when this was written: 11 366 to
12 830 correspondences each), set aside 0: the smallest margin on those batches is 2.5e-5 for the triangulation and
3.1e-4 for the last filter."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as entry  # noqa: E402
import two_view_verification_model as model  # noqa: E402
from oracle import oracle  # noqa: E402
from theiasfm_amd import abi, lib, synth  # noqa: E402

pytestmark = pytest.mark.gpu

MODELS = [(abi.PINHOLE, 0.4), (abi.PINHOLE_RADIAL_TANGENTIAL, 0.15), (abi.FISHEYE, 0.15), (abi.FOV, 0.15),
          (abi.DIVISION_UNDISTORTION, 0.15)]
MARGIN = 1e-9
CAP = 1e-3
OUT_KEYS = ("correspondence_status", "pair_status", "pair_num_verified", "termination", "iterations", "initial_cost",
            "final_cost")


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build_engine()
    entry.build_oracle()


def _options(**kw):
    return abi.two_view_verification_options(**kw)


def _set_aside(differ, margin, what):
    """The differing entries must all have a model margin below MARGIN, and be few."""
    n = int(differ.sum())
    print(f"{what}: {n} of {differ.size} set aside; smallest margin overall {margin.min():.3e}")
    assert (margin[differ] < MARGIN).all(), (what, margin[differ])
    assert n <= CAP * differ.size, (what, n)
    return n


@pytest.mark.parametrize("dof", [3, 4])
def test_staged_call_equals_fused_call_byte_for_byte(dof):
    """triangulate on the device (bundle_adjustment = 0), compact on the host, tmi_ba_adjust_two_views: the same bytes
    as the one call with bundle_adjustment = 1 -- the solve reads its survivors through corr_end and nothing else is
    different.  Free focal lengths on half of the pairs."""
    B, _ = synth.make_two_view_verification_batch(36, 40 + dof, models=MODELS, free_intrinsics=0.5)
    A = B.copy()
    tri = lib.verify_two_views(A, _options(bundle_adjustment=0), dof)
    assert set(tri["pair_status"]) == {0, 1, 2} and (tri["termination"] == -1).all()
    S, idx = model.compact(B, tri["correspondence_status"], A.points, tri["pair_status"])
    gated = tri["pair_status"] != 0
    assert (np.diff(S.correspondence_ptr)[gated] == 0).all() and gated.sum() >= 5
    term, iters, c0, c1, _ = lib.adjust_two_views(S, dof)
    F = B.copy()
    full = lib.verify_two_views(F, _options(), dof)
    assert term.tobytes() == full["termination"].tobytes()
    assert iters.tobytes() == full["iterations"].tobytes()
    assert c0.tobytes() == full["initial_cost"].tobytes() and c1.tobytes() == full["final_cost"].tobytes()
    assert (term[~gated] >= 0).all() and np.isin(term[~gated], (0, 1)).sum() >= 20
    assert S.extrinsics2.tobytes() == F.extrinsics2.tobytes()
    assert S.intrinsics1.tobytes() == F.intrinsics1.tobytes() and S.intrinsics2.tobytes() == F.intrinsics2.tobytes()
    assert (S.intrinsics1[:, 0] != B.intrinsics1[:, 0]).sum() >= 5  # focal lengths did move
    expect = A.points.copy()
    expect[idx] = S.points
    assert expect.tobytes() == F.points.tobytes()
    np.testing.assert_array_equal(F.extrinsics1, B.extrinsics1)


def test_triangulation_against_the_model():
    """Statuses equal (margin rule above; the model against itself in permuted order: 0 set aside, the triangulation is
    per correspondence), triangulated points to 1e-9 relative (the bound of test_gpu_estimate_tracks.py for the same
    triangulation), survivors per pair and pair statuses exact where nothing was set aside."""
    B, truth = synth.make_two_view_verification_batch(60, 51, models=MODELS, free_intrinsics=0.3)
    D = B.copy()
    D.points[:] = 7.25
    dev = lib.verify_two_views(D, _options(bundle_adjustment=0))
    M = B.copy()
    ref = model.verify(M, _options(bundle_adjustment=0))
    assert set(ref["correspondence_status"]) >= {-1, 0, 1, 3} and set(ref["pair_status"]) == {0, 1, 2}
    assert len(set(B.model1) | set(B.model2)) == 5
    differ = dev["correspondence_status"] != ref["correspondence_status"]
    _set_aside(differ, ref["margin"], "triangulation")
    both = (dev["correspondence_status"] == 0) & (ref["correspondence_status"] == 0)
    assert both.sum() > 0.6 * both.size
    scale = np.abs(M.points[both]).max(axis=1, keepdims=True)
    assert (np.abs(D.points[both] - M.points[both]) / scale).max() <= 1e-9
    assert (D.points[dev["correspondence_status"] != 0] == 7.25).all()  # untouched: the input is ignored, not cleared
    clean = np.add.reduceat(np.append(differ, False), B.correspondence_ptr[:-1]) == 0
    clean |= np.diff(B.correspondence_ptr) == 0
    np.testing.assert_array_equal(dev["pair_status"][clean], ref["pair_status"][clean])
    np.testing.assert_array_equal(dev["pair_num_verified"][clean], ref["pair_num_verified"][clean])
    s = dev["summary"]
    st = dev["correspondence_status"]
    assert s.num_pairs == 60 and s.num_correspondences == (st >= 0).sum()
    assert [s.num_verified, s.num_bad_triangulation_angles, s.num_failed_triangulations, s.num_bad_reprojection_errors,
            s.num_bad_final_reprojection_errors] == [(st == k).sum() for k in range(5)]
    assert [s.num_pairs_verified, s.num_pairs_too_few_matches, s.num_pairs_too_few_triangulated, s.num_pairs_failed_ba,
            s.num_pairs_too_few_verified] == [(dev["pair_status"] == k).sum() for k in range(5)]
    assert s.kernel_seconds > 0 and s.triangulate_kernel_seconds > 0 and s.solve_kernel_seconds == 0


@pytest.mark.parametrize("dof", [3, 4])
@pytest.mark.parametrize("free", [0.0, 0.5])
def test_solve_stage_against_the_oracle(dof, free):
    """oracle.adjust_two_views on the device's own compacted input, held to the bounds tests/test_two_view.py holds
    two_view_lm_kernel to: the pairs whose solve is short on both sides; point_dof 3: terminations and iteration counts
    equal, costs 1e-9, poses 1e-8, points 1e-6; point_dof 4: iteration counts within one, costs and poses 1e-5."""
    B, _ = synth.make_two_view_verification_batch(44, 60 + dof, models=MODELS, free_intrinsics=free)
    A = B.copy()
    tri = lib.verify_two_views(A, _options(bundle_adjustment=0), dof)
    R, idx = model.compact(B, tri["correspondence_status"], A.points, tri["pair_status"])
    term_o, it_o, c0_o, c1_o = oracle.adjust_two_views(R, dof)
    D = B.copy()
    dev = lib.verify_two_views(D, _options(), dof)
    term_d, it_d, c0_d, c1_d = dev["termination"], dev["iterations"], dev["initial_cost"], dev["final_cost"]
    np.testing.assert_allclose(c0_d, c0_o, rtol=1e-12, atol=1e-12)
    np.testing.assert_array_equal(term_d == -1, term_o == -1)
    short = (it_o <= 25) & (term_o >= 0)
    assert short.sum() >= 0.75 * (term_o >= 0).sum() and short.sum() >= 25
    rows = np.repeat(short, np.diff(R.correspondence_ptr))
    if dof == 3:
        np.testing.assert_array_equal(term_d[short], term_o[short])
        np.testing.assert_array_equal(it_d[short], it_o[short])
        np.testing.assert_allclose(c1_d[short], c1_o[short], rtol=1e-9)
        assert np.abs(D.points[idx[rows]] - R.points[rows]).max() <= 1e-7 * 10.0
        assert np.abs(D.extrinsics2[short] - R.extrinsics2[short]).max() <= 1e-8
        np.testing.assert_allclose(D.intrinsics2[short, 0], R.intrinsics2[short, 0], rtol=1e-9)
    else:
        np.testing.assert_array_equal(term_d[short] >= 2, term_o[short] >= 2)
        assert np.abs(it_d[short] - it_o[short]).max() <= 1
        np.testing.assert_allclose(c1_d[short], c1_o[short], rtol=1e-5)
        assert np.abs(D.extrinsics2[short] - R.extrinsics2[short]).max() <= 1e-5
    usable = np.isin(term_d, (0, 1))
    assert dev["summary"].total_iterations == it_d[term_d >= 0].sum()
    assert np.all(c1_d[usable] <= c0_d[usable] * (1 + 1e-12))
    assert (dev["pair_status"][(term_d >= 0) & ~usable] == 3).all()
    assert np.isin(dev["pair_status"][usable], (0, 4)).all()


@pytest.mark.parametrize("dof", [3, 4])
def test_final_filter_and_pair_status_against_the_model(dof):
    """Steps 5-6 of the model on the device's adjusted cameras and points (the model's permuted-order run on these
    seeds: 0 set aside).  Pair counts and statuses are exact wherever no correspondence of the pair was set aside."""
    B, truth = synth.make_two_view_verification_batch(60, 70 + dof, models=MODELS, free_intrinsics=0.3)
    A = B.copy()
    opts = _options()
    tri = lib.verify_two_views(A, _options(bundle_adjustment=0), dof)
    D = B.copy()
    dev = lib.verify_two_views(D, opts, dof)
    ran = np.isin(dev["termination"], (0, 1))
    np.testing.assert_array_equal(np.isin(dev["pair_status"], (0, 4)), ran)
    Cd, idx = model.compact(D, tri["correspondence_status"], D.points, tri["pair_status"])
    ok, margin = model.final_filter(Cd, opts, np.flatnonzero(ran))
    rows = np.repeat(ran, np.diff(Cd.correspondence_ptr))
    want = np.where(ok, 0, 4)[rows]
    got = dev["correspondence_status"][idx[rows]]
    assert set(got) == {0, 4} and (got == 4).sum() >= 20
    differ = got != want
    _set_aside(differ, margin[rows], "final filter")
    # everything else keeps the status of the triangulation
    rest = np.ones(B.features1.shape[0], dtype=bool)
    rest[idx[rows]] = False
    np.testing.assert_array_equal(dev["correspondence_status"][rest], tri["correspondence_status"][rest])
    moved = np.zeros(rest.size, dtype=bool)
    moved[idx[rows][differ]] = True
    for p in np.flatnonzero(ran):
        a, b = int(B.correspondence_ptr[p]), int(B.correspondence_ptr[p + 1])
        if moved[a:b].any():
            continue
        n = int(ok[Cd.correspondence_ptr[p]:Cd.correspondence_ptr[p + 1]].sum())
        assert dev["pair_num_verified"][p] == n == (dev["correspondence_status"][a:b] == 0).sum()
        assert dev["pair_status"][p] == (0 if n > opts.min_num_inlier_matches else 4)
    role = truth["role"]
    assert dev["pair_status"][role.index("end_min")] == 4 and dev["pair_num_verified"][role.index("end_min")] == 30
    assert dev["pair_status"][role.index("end_min_plus_1")] == 0
    assert dev["pair_num_verified"][role.index("end_min_plus_1")] == 31
    # cameras: written for the statuses 0 and 4, untouched otherwise
    np.testing.assert_array_equal(D.extrinsics2[~ran], B.extrinsics2[~ran])
    assert (D.extrinsics2[ran] != B.extrinsics2[ran]).any(axis=1).all()
    s = dev["summary"]
    assert s.solve_kernel_seconds > 0 and s.accept_kernel_seconds >= 0
    assert abs(s.triangulate_kernel_seconds + s.solve_kernel_seconds + s.accept_kernel_seconds - s.kernel_seconds) \
        <= 1e-6 + 1e-3 * s.kernel_seconds


def test_constructed_failed_adjustment_and_failed_triangulation():
    """The two statuses generated batches do not reach, on constructed pairs of plain pinhole cameras facing each other
    (tests/two_view_verification_model.py): pair 0 holds a survivor within 1e-4 of camera 1's centre, so its solve fails
    at the start point -- termination 3, PAIR status 3, correspondence statuses and points as the triangulation left
    them, cameras and (free) focal lengths untouched; pair 1 holds a correspondence on the common axis, whose
    antiparallel rays pass the angle test and make the midpoint system singular -- CORRESPONDENCE status 2; pair 2 is
    an ordinary pair with pixel noise, whose camera and focal lengths do move."""
    rng = np.random.default_rng(5)
    Xf = model.points(rng, 40, (3.0, 7.0)) - [0.5, 0, 0, 0]
    Xf[7] = [0.0, 0.0, 5.0, 1.0]
    side = model.noisy(model.mixed_pair(rng, 40, n_far=2)[0], rng)
    B = model.batch([model.failing_start_pair(rng), model.pair(model.E2_FACING, Xf), side])
    B.constant_intrinsics1[:] = 0
    B.constant_intrinsics2[:] = 0
    B.points[:] = 7.25
    for dof in (3, 4):
        T = B.copy()
        tri = lib.verify_two_views(T, _options(bundle_adjustment=0), dof)
        np.testing.assert_array_equal(tri["pair_status"], [0, 0, 0])
        want = np.zeros(122, dtype=np.int8)
        want[40 + 7] = 2
        want[120:] = 1
        np.testing.assert_array_equal(tri["correspondence_status"], want)
        assert tri["summary"].num_failed_triangulations == 1 and tri["summary"].num_bad_triangulation_angles == 2
        assert (T.points[want != 0] == 7.25).all()
        D = B.copy()
        dev = lib.verify_two_views(D, _options(), dof)
        M = B.copy()
        M.points[:] = 0
        ref = model.verify(M, _options(), dof)
        np.testing.assert_array_equal(ref["pair_status"], [3, 0, 0])
        np.testing.assert_array_equal(dev["pair_status"], [3, 0, 0])
        np.testing.assert_array_equal(dev["termination"], [3, 0, 0])
        np.testing.assert_array_equal(dev["pair_num_verified"], [40, 39, 40])
        assert dev["iterations"][0] == 0
        np.testing.assert_array_equal(dev["correspondence_status"], want)
        # the failed pair: points at the triangulated values, nothing of the cameras written
        assert D.points[:40].tobytes() == T.points[:40].tobytes()
        np.testing.assert_array_equal(D.extrinsics2[0], B.extrinsics2[0])
        np.testing.assert_array_equal(D.intrinsics1[0], B.intrinsics1[0])
        np.testing.assert_array_equal(D.intrinsics2[0], B.intrinsics2[0])
        assert (D.extrinsics2[2] != B.extrinsics2[2]).any() and (D.intrinsics1[2, 0] != B.intrinsics1[2, 0])
        s = dev["summary"]
        assert s.num_pairs_failed_ba == 1 and s.num_pairs_verified == 2 and s.num_failed_triangulations == 1


def _one_pair(B, p):
    a, b = int(B.correspondence_ptr[p]), int(B.correspondence_ptr[p + 1])
    return abi.TwoViewBatch(B.extrinsics1[p:p + 1].copy(), B.extrinsics2[p:p + 1].copy(), B.model1[p:p + 1].copy(),
                            B.model2[p:p + 1].copy(), B.intrinsics1[p:p + 1].copy(), B.intrinsics2[p:p + 1].copy(),
                            B.constant_intrinsics1[p:p + 1].copy(), B.constant_intrinsics2[p:p + 1].copy(),
                            np.array([0, b - a], dtype=np.int64), B.features1[a:b].copy(), B.features2[a:b].copy(),
                            B.points[a:b].copy()), a, b


@pytest.mark.parametrize("dof", [3, 4])
def test_every_pair_alone_gives_the_bytes_of_the_batch(dof):
    """A pair's result depends on the pair alone: 40 pairs (63, 64 and 65 correspondences, gated pairs, an empty pair)
    in one call and each in a call of its own."""
    counts = np.random.default_rng(3).integers(40, 300, 40)
    counts[20] = 0
    counts[[7, 8, 9]] = [63, 64, 65]  # (the generator's n63 / n64 / n65 pairs take their size from counts)
    B, truth = synth.make_two_view_verification_batch(40, 80 + dof, models=MODELS, free_intrinsics=0.4, counts=counts)
    n = np.diff(B.correspondence_ptr)
    assert n[20] == 0 and {63, 64, 65} <= set(n.tolist())
    B.points[:] = 7.25
    D = B.copy()
    dev = lib.verify_two_views(D, _options(), dof)
    assert dev["pair_status"][20] == 1 and set(dev["pair_status"]) >= {0, 1, 2, 4}
    for p in range(B.num_pairs):
        one, a, b = _one_pair(B, p)
        r = lib.verify_two_views(one, _options(), dof)
        assert r["correspondence_status"].tobytes() == dev["correspondence_status"][a:b].tobytes(), p
        for k in OUT_KEYS[1:]:
            assert r[k].tobytes() == dev[k][p:p + 1].tobytes(), (p, k)
        for f in ("extrinsics2", "intrinsics1", "intrinsics2"):
            assert getattr(one, f).tobytes() == getattr(D, f)[p:p + 1].tobytes(), (p, f)
        assert one.points.tobytes() == D.points[a:b].tobytes(), p


def test_outputs_may_be_null_and_repeat_runs_agree():
    B, _ = synth.make_two_view_verification_batch(16, 90, models=MODELS)
    D1, D2, D3 = B.copy(), B.copy(), B.copy()
    r1 = lib.verify_two_views(D1, _options())
    r2 = lib.verify_two_views(D2, _options())
    for k in OUT_KEYS:
        assert r1[k].tobytes() == r2[k].tobytes(), k
    assert D1.points.tobytes() == D2.points.tobytes() and D1.extrinsics2.tobytes() == D2.extrinsics2.tobytes()
    L = lib.load()
    cb = D3.as_c()
    s = abi.CTwoViewVerificationSummary()
    o = _options()
    assert L.tmi_ba_verify_two_views(C.byref(cb), C.byref(o), 4, 200, -1, None, None, None, None, None, None, None,
                                     C.byref(s)) == 0
    assert D3.points.tobytes() == D1.points.tobytes() and D3.extrinsics2.tobytes() == D1.extrinsics2.tobytes()
    assert s.num_pairs_verified == (r1["pair_status"] == 0).sum() and s.num_pairs == 16
    # no pairs at all
    E = abi.TwoViewBatch(np.zeros((0, 6)), np.zeros((0, 6)), [], [], np.zeros((0, 10)), np.zeros((0, 10)), [], [],
                         np.zeros(1, np.int64), np.zeros((0, 2)), np.zeros((0, 2)), np.zeros((0, 4)))
    r = lib.verify_two_views(E, _options())
    assert r["pair_status"].size == 0 and r["summary"].num_pairs == 0
