"""-m gpu: tmi_ba_optimize_relative_positions (relative_position_kernels.h) against the CPU model
(tests/relative_position_model.py).

"Device equals model" on a direction means an angle (atan2 form) of at most max(1e-12 rad, 100 x MODEL_SPREAD), with
MODEL_SPREAD the largest angle between two runs of the MODEL on the same batch -- SVD / natural order against eigh / a
permuted order.  The device differs from the model in exactly those two ways (another 3 x 3 eigen-solver, another
summation order), and 100 x is the margin the project gives round-off elsewhere.  Costs: rtol 1e-9.  A pair whose
iteration count differs from the model's by exactly one is set aside from the direction comparison (the stopping test
compares a round-off sized change with 1e-5); at most 2 % of the pairs may be.  The raw sign of an eigenvector is the
implementation's own: nothing here assumes which way the vector pointed before the flip.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as entry  # noqa: E402
import relative_position_model as model  # noqa: E402
from oracle import oracle  # noqa: E402
from theiasfm_amd import abi, lib, synth  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 7.25
ALL_MODELS = [(abi.PINHOLE, 0.2), (abi.PINHOLE_RADIAL_TANGENTIAL, 0.2), (abi.FISHEYE, 0.2), (abi.FOV, 0.2),
              (abi.DIVISION_UNDISTORTION, 0.2)]
# sizes around the wavefront width and around the register cap of the kernel (8 columns per lane: 512)
SPECIAL_SIZES = (8, 20, 63, 64, 65, 200, 511, 512, 513, 700, 2500)


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build_engine()
    entry.build_oracle()


def _run(B):
    B.position2[:] = SENTINEL
    return lib.optimize_relative_positions(B)


def _counts(n_pairs, seed):
    rng = np.random.default_rng(seed)
    special = np.repeat(SPECIAL_SIZES, 6)
    return rng.permutation(np.concatenate([special, rng.integers(8, 601, n_pairs - len(special))]))


def _compare(B, normalise, what):
    res, spread, count_diff, ambiguous = model.model_spread(B, normalise)
    assert ambiguous == 0 and count_diff == 0, (ambiguous, count_diff)
    tol = max(1e-12, 100.0 * spread)
    D = B.copy()
    status, iters, cost, front, ts = _run(D)
    n = np.diff(B.correspondence_ptr)
    aside, worst, worst_cost = 0, 0.0, 0.0
    bad = []
    for p, r in enumerate(res):
        if status[p] != r.status or front[p] != r.num_in_front or not front[p] > n[p] // 2:
            bad.append((p, int(n[p]), int(status[p]), r.status, int(front[p]), r.num_in_front))
            continue
        if abs(int(iters[p]) - r.iterations) == 1:
            aside += 1
            continue
        if iters[p] != r.iterations:
            bad.append((p, int(n[p]), "iterations", int(iters[p]), r.iterations))
            continue
        a = model.angle(D.position2[p], r.t)          # includes the sign: a flipped vector is an angle of pi
        worst = max(worst, a)
        worst_cost = max(worst_cost, abs(cost[p] - r.cost) / max(abs(r.cost), 1e-300))
    print(f"{what}: {B.num_pairs} pairs, MODEL_SPREAD {spread:.3e} rad, tolerance {tol:.3e} rad, device-to-model max "
          f"{worst:.3e} rad, cost max rel {worst_cost:.3e}, set aside {aside}, iterations {iters.min()}..{iters.max()}, "
          f"kernel {ts.kernel_seconds * 1e3:.3f} ms")
    assert not bad, bad[:10]
    assert aside <= 0.02 * B.num_pairs
    assert worst <= tol
    assert worst_cost <= 1e-9
    assert abs(np.linalg.norm(D.position2, axis=1) - 1.0).max() < 1e-12


def test_reference_cases_on_the_device():
    """The reference's four tests (optimize_relative_position_with_known_rotation_test.cc:127-219) on the seed lists of
    the CPU test: the device meets the reference's bounds."""
    for name, noise, seeds, bound in model.REFERENCE_CASES:
        rot, f1, f2, truth = [], [], [], []
        for seed in seeds:
            a, b, r1, r2, t = model.reference_test_case(seed, noise)
            rot += [r1, r2]
            f1.append(a)
            f2.append(b)
            truth.append(t)
        P = len(seeds)
        B = abi.RelativePositionBatch(np.array(rot), np.arange(P) * 2, np.arange(P) * 2 + 1, np.arange(P + 1) * 100,
                                      np.concatenate(f1), np.concatenate(f2))
        status, iters, cost, front, _ = _run(B)
        deg = np.degrees([model.angle(B.position2[p], truth[p]) for p in range(P)])
        print(f"{name}: max {deg.max():.3e} deg (bound {bound}), iterations {iters.min()}..{iters.max()}")
        assert (status == 0).all() and (front > 50).all()
        assert (deg < bound).all(), (name, deg)


def test_batch_of_normalised_features_equals_the_model():
    B, _ = synth.make_relative_position_batch(2000, 21, pixel_noise=0.5, counts=_counts(2000, 21))
    _compare(B, None, "normalised")


def test_batch_of_pixels_equals_the_model():
    B, _ = synth.make_relative_position_batch(600, 22, pixel_noise=0.5, counts=_counts(600, 22), models=ALL_MODELS)
    assert set(B.view_model.tolist()) == {0, 1, 2, 3, 4}

    def normalise(v, px):
        pt = oracle.pixel_to_camera_batch(int(B.view_model[v]), B.view_intrinsics[v], px)
        return pt[:, :2] / pt[:, 2:3]

    _compare(B, normalise, "pixels")


def _two_views(n_front, n_behind, seed, baseline=(1.0, 0.1, 0.0)):
    """Exact correspondences of two views (view 1 at the origin): n_front points in front of both, n_behind BEHIND both,
    projected all the same (x / z, y / z)."""
    rng = np.random.default_rng(seed)
    r1, r2 = 0.1 * rng.uniform(-1, 1, 3), 0.1 * rng.uniform(-1, 1, 3)
    C2 = np.asarray(baseline, dtype=np.float64)
    z = np.concatenate([rng.uniform(4, 8, n_front), -rng.uniform(4, 8, n_behind)])
    X = np.stack([rng.uniform(-1, 1, len(z)), rng.uniform(-1, 1, len(z)), z], 1) @ model.aa_to_R(r1)  # world
    q1, q2 = X @ model.aa_to_R(r1).T, (X - C2) @ model.aa_to_R(r2).T
    assert (np.sign(q1[:, 2]) == np.sign(z)).all() and (np.sign(q2[:, 2]) == np.sign(z)).all()
    return r1, r2, q1[:, :2] / q1[:, 2:3], q2[:, :2] / q2[:, 2:3]


def test_built_cases():
    pairs = [
        _two_views(0, 0, 1),                                 # 0 empty
        _two_views(12, 0, 2),                                # 1 NaN features
        _two_views(1, 0, 3),                                 # 2 one correspondence
        _two_views(2, 0, 4),                                 # 3 two correspondences
        _two_views(40, 0, 5, baseline=(0.0, 0.0, 0.0)),      # 4 zero baseline
        _two_views(30, 30, 6),                               # 5 neither sign has a majority
        _two_views(50, 0, 7),                                # 6 an ordinary pair next to them
    ]
    pairs[1][2][3, 1] = np.nan
    rot = np.array([r for q in pairs for r in q[:2]])
    ptr = np.concatenate([[0], np.cumsum([len(q[2]) for q in pairs])])
    B = abi.RelativePositionBatch(rot, np.arange(7) * 2, np.arange(7) * 2 + 1, ptr,
                                  np.concatenate([q[2] for q in pairs]), np.concatenate([q[3] for q in pairs]))
    status, iters, cost, front, ts = _run(B)
    print("status", status, "iterations", iters, "in front", front, "cost", cost)
    sentinel = np.full(3, SENTINEL).tobytes()
    assert status[0] == -1 and B.position2[0].tobytes() == sentinel
    assert status[1] == 2 and B.position2[1].tobytes() == sentinel
    for p in (2, 3, 4):
        assert status[p] in (0, 1)
        assert np.isfinite(B.position2[p]).all() and abs(np.linalg.norm(B.position2[p]) - 1.0) < 1e-12
    r = model.solve(pairs[5][2], pairs[5][3], pairs[5][0], pairs[5][1])
    assert r.ambiguous and r.front_plus == 30 and r.front_minus == 30
    assert status[5] == r.status and front[5] == 60 // 2
    a = model.angle(B.position2[5], r.t)
    assert min(a, np.pi - a) < 1e-9, a                       # equal UP TO SIGN
    r6 = model.solve(pairs[6][2], pairs[6][3], pairs[6][0], pairs[6][1])
    assert status[6] == 0 and front[6] == 50 and model.angle(B.position2[6], r6.t) < 1e-9
    # summary: pairs with correspondences, pairs with a position
    assert ts.num_tracks == 6 and ts.num_success == 5 and ts.kernel_seconds > 0
    assert ts.total_iterations == int(iters.sum())


def test_runs_are_bit_reproducible_and_pairs_independent():
    counts = np.concatenate([np.repeat((8, 63, 64, 65, 511, 512, 513, 700, 2500), 2),
                             np.random.default_rng(5).integers(8, 400, 19)])
    assert len(counts) == 37
    B, _ = synth.make_relative_position_batch(37, 31, pixel_noise=0.5, counts=counts, models=ALL_MODELS)
    A1, A2 = B.copy(), B.copy()
    o1, o2 = _run(A1), _run(A2)
    assert A1.position2.tobytes() == A2.position2.tobytes()
    for a, b in zip(o1[:4], o2[:4]):
        assert a.tobytes() == b.tobytes()
    assert (o1[0] == 0).all()
    # four pairs share a workgroup: every pair alone gives the bytes it gave inside the batch
    for p in range(37):
        S = B.pair(p)
        s = _run(S)
        assert S.position2[0].tobytes() == A1.position2[p].tobytes(), p
        for a, b in zip(s[:4], o1[:4]):
            assert a[0].tobytes() == b[p].tobytes(), p
    # optional outputs: NULL for all of them
    import ctypes as C
    N = B.copy()
    ts = abi.CTrackBatchSummary()
    assert lib.load().tmi_ba_optimize_relative_positions(C.byref(N.as_c()), -1, None, None, None, None,
                                                         C.byref(ts)) == 0
    assert N.position2.tobytes() == A1.position2.tobytes() and ts.num_success == 37
