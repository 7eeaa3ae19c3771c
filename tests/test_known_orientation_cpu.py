"""The two known-orientation position RANSACs without a device: the numpy model (tests/known_orientation_model.py)
restates the reference's eight estimator tests and the solver tests of position_from_two_rays_test.cc /
relative_pose_from_two_points_with_known_rotation_test.cc; its closed path against its numpy path; its decision margins
on the GPU tests' inputs (tests/known_orientation_cases.py); the C ABI's argument errors; the C++ shim's refusals and
no-device behaviour (tests/cpp/test_known_orientation_shim.cc, compiled here)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import known_orientation_cases as cases  # noqa: E402
import known_orientation_model as model  # noqa: E402
from shim_build import compile_shim  # noqa: E402
from theiasfm_amd import abi, lib  # noqa: E402

NO_DEVICE = dict(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
SCORINGS = [False, True]
# the largest relative difference between the closed path and the numpy path (lstsq / SVD) over the 225 samples of
# _path_rows() per problem, none of which has a flagged rank margin, MEASURED: 7.75e-15 (absolute), 1.32e-14 (relative).
# The assertion is at PATH_FACTOR = 16 times that.
PATH_MEASURED = {"absolute": 7.75e-15, "relative": 1.32e-14}
PATH_FACTOR = 16.0


def _solver_rows(kind):
    """The solver tests' two-point samples as rows of the problem's planes, with the true position."""
    out = []
    for pts, pos in cases.solver_cases(kind):
        X, pos = np.array(pts).reshape(2, 3), np.array(pos)
        f2 = (X - pos)[:, :2] / (X - pos)[:, 2:]
        if kind == "absolute":
            rows = [[float(f2[k, 0]), float(f2[k, 1])] + [float(t) for t in X[k]] for k in range(2)]
        else:
            f1 = X[:, :2] / X[:, 2:]
            rows = [[float(f1[k, 0]), float(f1[k, 1]), float(f2[k, 0]), float(f2[k, 1])] for k in range(2)]
        out.append((rows, pos))
    return out


def _path_rows(kind):
    """The solver tests' samples and every sample the model replays on the main batch."""
    rows = [r for r, _ in _solver_rows(kind)]
    m, b = cases.main_model(kind, True), cases.main_batch(kind)
    po = b["item_offset"]
    for p, r in m["results"].items():
        a = int(po[p])
        for i in r.hyp:
            s = model.sample(cases.MAIN_RANSAC_SEED, p, i, r.n)
            pair = []
            for k in s:
                v = [float(t) for rot in m["rotated"] for t in rot[a + k]]
                pair.append(v + ([float(t) for t in b["world_point"][a + k]] if kind == "absolute" else []))
            rows.append(pair)
    return rows


def _path_difference(kind, closed, numpy_):
    a, b = np.array(closed), np.array(numpy_)
    if kind == "absolute":
        return float(np.abs(a - b).max() / max(np.abs(b).max(), 1.0))
    return float(min(np.abs(a - b).max(), np.abs(a + b).max()))  # unit vectors; the sign is not part of the estimate


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("variant", range(4))
def test_reference_estimator_tests(kind, variant):
    """estimate_absolute_pose_with_known_orientation_test.cc:127-240 and
    estimate_relative_pose_with_known_orientation_test.cc:124-237, all with use_mle: 100 points, a 4 px threshold at
    focal 1000, failure probability 0.001; success (:110, :108), more than 3 inliers (:118, :115) and
    ArraysEqualUpToScale within kPoseTolerance (:121-124, :118-121) = 1e-4 (AllInliersNoNoise), 1e-2 (the others)."""
    b, m = cases.reference_batch(kind), cases.reference_model(kind)
    items = range(0, 6) if variant == 0 else range(6, 12) if variant == 1 else range(12 + 4 * (variant - 2), 16 + 4 * (variant - 2))
    ratio, _, tolerance, _ = cases.REFERENCE_VARIANTS[variant]
    for p in items:
        assert b["tolerance"][p] == tolerance
        assert m["status"][p] == 0 and m["num_inliers"][p] > 3
        assert model.direction_difference(m["position"][p], b["position"][p]) <= tolerance, p
        assert m["num_iterations"][p] >= 100
        if ratio == 1.0 and variant == 0:
            assert m["num_inliers"][p] == cases.REFERENCE_POINTS


@pytest.mark.parametrize("path", ["closed", "numpy"])
@pytest.mark.parametrize("kind", cases.KINDS)
def test_reference_solver_tests(kind, path):
    """BasicTest, DifferentAxesTest and ManyPointsTest of position_from_two_rays_test.cc:156-220 and
    relative_pose_from_two_points_with_known_rotation_test.cc:148-212, all without noise: the solver succeeds and the
    position (the unit direction) is within kTolerance = 1e-4 (:67, :99 / :91).  The reference compares the direction
    WITH its sign, which is FullPivLU's; here the sign is not part of the estimate and the comparison is up to sign."""
    solve = model.PROBLEMS[kind][0]
    for rows, pos in _solver_rows(kind):
        h = solve(rows, path)
        assert h.ok and h.margins["rank"] > 1e6
        if kind == "absolute":
            assert np.linalg.norm(np.array(h.model) - pos) < cases.SOLVER_TOLERANCE
        else:
            t = pos / np.linalg.norm(pos)
            assert min(np.linalg.norm(np.array(h.model) - t), np.linalg.norm(np.array(h.model) + t)) < cases.SOLVER_TOLERANCE


@pytest.mark.parametrize("kind", cases.KINDS)
def test_closed_path_against_numpy_path(kind):
    solve = model.PROBLEMS[kind][0]
    worst, used = 0.0, 0
    for rows in _path_rows(kind):
        c, n = solve(rows, "closed"), solve(rows, "numpy")
        assert c.ok == n.ok
        if c.margins["rank"] < model.MARGIN or not c.ok:
            continue
        worst = max(worst, _path_difference(kind, c.model, n.model))
        used += 1
    print(f"{kind}: closed - numpy worst {worst:.3e} over {used} samples (measured {PATH_MEASURED[kind]:.3e})")
    assert used >= 200
    # measured 7.75e-15 (absolute) / 1.32e-14 (relative); asserted at 16 x the measured value
    assert worst <= PATH_FACTOR * PATH_MEASURED[kind]


def test_degenerate_samples_give_no_model():
    """Equal rotated features (the 4x3 system has rank 2), a pair without baseline and a repeated correspondence (the
    2x3 matrix has rank 0 / 1): no model, the margin far on the rank-deficient side."""
    h = model.position_from_two_rays([[0.125, -0.0625, 1.0, 2.0, 8.0], [0.125, -0.0625, 2.0, 1.0, 9.0]])
    assert not h.ok and h.reason == "rank" and h.margins["rank"] == 1.0
    h = model.relative_position_from_two_points([[0.1, 0.2, 0.1, 0.2], [-0.3, 0.05, -0.3, 0.05]])
    assert not h.ok and h.reason == "rank" and h.margins["rank"] == 1.0
    h = model.relative_position_from_two_points([[0.1, 0.2, 0.15, 0.22], [0.1, 0.2, 0.15, 0.22]])
    assert not h.ok and h.reason == "rank" and h.margins["rank"] == 1.0
    # the sign rule: swapping the two rows negates the direction exactly, and the residuals do not see it
    a = model.relative_position_from_two_points([[0.1, 0.2, 0.15, 0.22], [-0.3, 0.05, -0.2, 0.07]])
    b = model.relative_position_from_two_points([[-0.3, 0.05, -0.2, 0.07], [0.1, 0.2, 0.15, 0.22]])
    assert a.ok and b.ok and a.model == [-t for t in b.model]
    P = [np.array([0.3, -0.2]), np.array([0.1, 0.4]), np.array([0.25, -0.1]), np.array([0.12, 0.45])]
    assert model.sampson_residuals(a.model, P).tobytes() == model.sampson_residuals(b.model, P).tobytes()


@pytest.mark.parametrize("kind", cases.KINDS)
def test_rotation_by_zero_passes_the_features_through(kind):
    f = cases.main_batch(kind)["features"][0]
    assert model.rotate(f, np.zeros(3)).tobytes() == f.tobytes()


@pytest.mark.parametrize("name,use_mle", [("main", False), ("main", True), ("planted", False), ("planted", True),
                                          ("reference", True)])
@pytest.mark.parametrize("kind", cases.KINDS)
def test_margins_on_the_gpu_tests_inputs(kind, name, use_mle):
    """At most 1 % of the hypotheses with a model are flagged (a condition of tests/test_gpu_known_orientation.py), and
    no flagged hypothesis is a best model or changes a bound.  (The reference's scenes run with use_mle only.)"""
    m = {"main": lambda: cases.main_model(kind, use_mle), "planted": lambda: cases.planted_model(kind, use_mle),
         "reference": lambda: cases.reference_model(kind)}[name]()
    total = int(np.count_nonzero(m["hypothesis_cost"] >= 0))
    flagged = int(np.count_nonzero(m["flagged"]))
    print(f"{kind} {name} use_mle={use_mle}: {flagged} of {total} flagged")
    assert total > 0 and flagged <= 0.01 * total
    for p, r in m["results"].items():
        assert r.best_iteration not in r.flagged and not (r.bound_changers & r.flagged)


@pytest.mark.parametrize("kind", cases.KINDS)
def test_main_batch_is_what_the_gpu_test_expects(kind):
    for use_mle in SCORINGS:
        m = cases.main_model(kind, use_mle)
        assert m["status"].tolist() == [0, 0, 0, 0, 0, 0, 1, -1, 2, 0]
        assert m["num_iterations"][cases.DEGENERATE_ITEM] == cases.MAX_ITERATIONS
        for r in (m["results"][cases.DEGENERATE_ITEM],):
            assert all(h.reason == "rank" and h.margins["rank"] == 1.0 for h in r.hyp.values())
        q = cases.OUTLIER_ITEM
        assert model.direction_difference(m["position"][q], cases.main_batch(kind)["position"][q]) <= 1e-2
    # the two scorings differ
    p = cases.MLE_ITEM[kind]
    assert cases.main_model(kind, False)["best_iteration"][p] != cases.main_model(kind, True)["best_iteration"][p]


@pytest.mark.parametrize("use_mle", SCORINGS)
@pytest.mark.parametrize("kind", cases.KINDS)
def test_chunked_replay_equals_the_reference_loop(kind, use_mle):
    a = cases.main_model(kind, use_mle)
    for chunk in (1, 7):
        b = cases.main_model(kind, use_mle, "closed", chunk)
        for k in ("status", "num_inliers", "num_iterations", "best_iteration", "corr_inlier", "hypothesis_cost"):
            assert np.array_equal(a[k], b[k]), (chunk, k)
        assert a["position"].tobytes() == b["position"].tobytes()
        assert a["hypothesis_cost_real"].tobytes() == b["hypothesis_cost_real"].tobytes()


def test_ransac_sample_of_two_matches_the_models_sampler(tmp_path):
    """ransac_sample<2> of theiasfm_amd/csrc/ransac_core.h, compiled for the host under -fsanitize=address,undefined
    (tests/cpp/ransac_sample2_host_check.cc: its own main), as tests/test_homography_cpu.py does for 4."""
    import itertools

    import __graft_entry__ as entry
    exe = str(tmp_path / "ransac_sample2_host_check")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    cmd = [entry._hipcc(), "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", *san,
           "-I" + os.path.join(ROOT, "theiasfm_amd", "csrc"), "-o", exe,
           os.path.join(ROOT, "tests", "cpp", "ransac_sample2_host_check.cc")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr
    inputs = [(seed, stream, i, n) for n in (2, 3, 65, 1000)
              for seed, stream, i in itertools.product((0, 0x9E3779B97F4A7C15), (0, 1, 2**32 - 1), (0, 1, 2**20 - 1))]
    text = "".join("%d %d %d %d\n" % c for c in inputs)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", **NO_DEVICE)
    p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, p.stderr
    lines = p.stdout.splitlines()
    assert len(lines) == len(inputs)
    for (seed, stream, i, n), line in zip(inputs, lines):
        want = tuple(model.sample(seed, stream, i, n))
        assert tuple(map(int, line.split())) == want, (seed, stream, i, n)
        assert len(set(want)) == 2 and all(0 <= k < n for k in want)


def _lib_call(kind, b, th, **kw):
    if kind == "absolute":
        args = dict(item_offset=b["item_offset"], feature=b["features"][0], world_point=b["world_point"],
                    item_orientation=b["orientations"][0], item_error_threshold=th)
        fn = lib.estimate_positions_known_orientation
        rename = {}
    else:
        args = dict(pair_offset=b["item_offset"], feature1=b["features"][0], feature2=b["features"][1],
                    pair_orientation1=b["orientations"][0], pair_orientation2=b["orientations"][1],
                    pair_error_threshold=th)
        fn = lib.estimate_relative_positions_known_orientation
        rename = dict(item_offset="pair_offset", item_error_threshold="pair_error_threshold", item_mask="pair_mask")
    args["options"] = abi.known_orientation_ransac_options(**cases.KW)
    args.update({rename.get(k, k): v for k, v in kw.items()})
    return fn(**args)


@pytest.mark.parametrize("kind", cases.KINDS)
def test_argument_errors(kind):
    """Returned before the device is looked for, so they need none."""
    b = cases.planted_batch(kind)
    sm = b["samples"]
    th = np.full(3, cases.THRESHOLD)

    def status(**kw):
        with pytest.raises(lib.EngineError) as e:
            _lib_call(kind, b, th, **kw)
        return e.value.status

    for wrong in ((4, 4), (2, 30), (-1, 0)):  # repeated, out of range
        bad = sm.copy()
        bad[1, 7] = wrong
        assert status(samples=bad) == abi.ERR_INVALID_ARGUMENT
    assert status(item_error_threshold=np.array([4e-6, 0.0, 4e-6])) == abi.ERR_INVALID_ARGUMENT
    assert status(item_error_threshold=np.array([4e-6, np.nan, 4e-6])) == abi.ERR_INVALID_ARGUMENT
    assert status(item_offset=np.array([0, 30, 20, 65])) == abi.ERR_INVALID_ARGUMENT
    assert status(item_offset=np.array([1, 30, 60, 65])) == abi.ERR_INVALID_ARGUMENT
    for kw in (dict(failure_probability=0.0), dict(failure_probability=1.0), dict(min_inlier_ratio=1.5),
               dict(min_iterations=65, max_iterations=64), dict(max_iterations=(1 << 20) + 1),
               dict(chunk_iterations=-1)):
        for mle in (0, 1):
            assert status(options=abi.known_orientation_ransac_options(use_mle=mle, **kw)) == abi.ERR_INVALID_ARGUMENT, kw
    # the real costs exist under MLE only
    assert status(want_hypothesis_cost_real=True) == abi.ERR_INVALID_ARGUMENT
    # a bad sample of an item that is NOT attempted (masked out) is not looked at: the call gets as far as the device
    bad = sm.copy()
    bad[1, 7] = (4, 4)
    try:
        _lib_call(kind, b, th, item_mask=[1, 0, 1], samples=bad)
    except lib.EngineError as e:
        assert e.status != abi.ERR_INVALID_ARGUMENT


def test_null_arguments():
    """The raw entry points: null options or summary, a null offset array, missing orientations."""
    L = lib.load()
    o = abi.known_orientation_ransac_options()
    s = abi.CTwoViewRansacSummary()
    import ctypes as C
    zero = np.zeros(2, dtype=np.int64)
    for fn, nptr in ((L.tmi_ba_estimate_positions_known_orientation, 8),
                     (L.tmi_ba_estimate_relative_positions_known_orientation, 9)):
        nout = 11 if nptr == 8 else 12
        rest = [None] * (nptr - 1) + [0] + [None] * nout
        assert fn(None, 0, zero.ctypes.data, *rest, C.byref(s)) == abi.ERR_INVALID_ARGUMENT
        assert fn(C.byref(o), 0, zero.ctypes.data, *rest, None) == abi.ERR_INVALID_ARGUMENT
        assert fn(C.byref(o), 0, None, *rest, C.byref(s)) == abi.ERR_INVALID_ARGUMENT
        assert fn(C.byref(o), -1, zero.ctypes.data, *rest, C.byref(s)) == abi.ERR_INVALID_ARGUMENT
        # one item without correspondences, but no orientation array
        assert fn(C.byref(o), 1, zero.ctypes.data, *rest, C.byref(s)) == abi.ERR_INVALID_ARGUMENT


def _compile(tmp_path, extra=()):
    return compile_shim(tmp_path, "test_known_orientation_shim.cc",
                        ["known_orientation_ops.cc", "localize_ops.cc", "view_ops.cc", "bundle_adjuster.cc"], extra)


def test_shim_without_a_device(tmp_path):
    p = subprocess.run([_compile(tmp_path)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, **NO_DEVICE))
    print(p.stdout, p.stderr)
    assert p.returncode == 0 and "known orientation shim: OK" in p.stdout, p.stdout + p.stderr
    assert "unsupported: only RansacType::RANSAC" in p.stderr


def test_shim_under_host_sanitizers(tmp_path):
    """The stand-alone program with -fsanitize=address,undefined on the shim and the test (the engine library is not
    instrumented).  Leak checking is off: the HIP runtime's start-up allocations are not the shim's."""
    exe = _compile(tmp_path,
                   ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", **NO_DEVICE)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    print(p.stdout, p.stderr)
    assert p.returncode == 0 and "known orientation shim: OK" in p.stdout, p.stdout + p.stderr


@pytest.mark.gpu
def test_shim_on_the_device(tmp_path):
    p = subprocess.run([_compile(tmp_path), "--need-device"], capture_output=True, text=True, timeout=600)
    print(p.stdout, p.stderr)
    assert p.returncode == 0 and "known orientation shim: OK (device)" in p.stdout, p.stdout + p.stderr
