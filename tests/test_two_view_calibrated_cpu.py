"""The numpy model of tmi_ba_estimate_calibrated_relative_poses (tests/two_view_calibrated_model.py) on its own, the
conditions tests/test_gpu_two_view_calibrated.py relies on, and the kernels' own text on the host -- no device:
  flags     on exactly the GPU test's inputs at most 2 % of the replayed samples are flagged, none of them a best model
            or a sample that lowers the bound
  coverage  statuses 0, 1, 2; three different real-root counts; a sample with fewer models than real roots; a sample
            without a model
  paths     the closed and the numpy path agree on every unflagged decision
  solver    five_point_relative_pose_test.cc:115-190: every solution's Sampson distance on its five points below 1e-8,
            one solution equal to the true E up to scale (the reference's cosine test and per-case tolerances)
  ransac    estimate_relative_pose_test.cc:141-163 (all inliers, no noise): rotation and translation direction within
            1e-4 degrees
  host      steps 3 and 4 of two_view_calibrated_kernels.h compiled for the host (stride-1 slab, its own main, under
            -fsanitize=address,undefined) give the closed path's bits
  errors    argument errors come before the device is looked for"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402
import two_view_calibrated_cases as cases  # noqa: E402
import two_view_calibrated_model as model  # noqa: E402
from theiasfm_amd import abi, lib, synth  # noqa: E402


def _lists(x1, x2):
    return [list(map(float, v)) for v in (x1[:, 0], x1[:, 1], x2[:, 0], x2[:, 1])]


def test_flag_cap_on_the_gpu_tests_inputs():
    replayed = flagged = 0
    for m in (cases.main_model(), cases.planted_model()):
        for p, r in m["results"].items():
            replayed += len(r.hyp)
            flagged += len(r.flagged)
            assert r.best_iteration not in r.flagged, (p, r.best_iteration)
            assert not (r.flagged & r.bound_changers), (p, r.flagged & r.bound_changers)
    print(f"replayed {replayed} flagged {flagged}")
    assert replayed > 300 and flagged <= 0.02 * replayed


def test_coverage_of_the_inputs():
    main, planted = cases.main_model(), cases.planted_model()
    assert {0, 1} <= set(main["status"].tolist()) and 2 in planted["status"].tolist()
    hyps = [h for m in (main, planted) for r in m["results"].values() for h in r.hyp.values()]
    roots = {h.num_real_roots for h in hyps if h.num_real_roots}
    print("real-root counts", sorted(roots))
    assert len(roots) >= 3
    assert any(0 < len(h.models) < h.num_real_roots for h in hyps)
    assert any(not h.ok for h in hyps)
    # the planted samples: a duplicated correspondence, an all-degenerate pair, forward motion, no rotation
    assert planted["results"][0].hyp[0].reason == "rank5" and planted["hypothesis_cost"][0, 0].max() == -1
    assert all(h.reason == "rank5" for h in planted["results"][1].hyp.values())
    assert planted["num_iterations"][1] == cases.MAX_ITERATIONS and planted["best_iteration"][1] == -1
    for p in (2, 3):
        assert planted["status"][p] == 0 and planted["best_iteration"][p] == 0
        assert planted["num_inliers"][p] == 40 and 0 in planted["hypothesis_cost"][p, 0]


def test_the_two_paths_agree_on_unflagged_decisions():
    a, b = cases.main_model(), cases.main_model("numpy")
    ok = ~a["flagged"] & ~b["flagged"]
    assert np.array_equal(a["hypothesis_cost"][ok], b["hypothesis_cost"][ok])
    for k in ("status", "num_inliers", "num_iterations", "best_iteration", "best_solution", "corr_inlier"):
        assert np.array_equal(a[k], b[k]), k
    spread = model.model_spread(a, b)
    print(f"MODEL_SPREAD {spread:.3e}")
    assert spread < 1e-9
    c = cases.main_model(chunk=5)
    for k in ("status", "num_inliers", "num_iterations", "best_iteration", "best_solution", "essential_matrix"):
        assert np.array_equal(a[k], c[k]), k


@pytest.mark.parametrize("name", sorted(cases.FIXTURES))
@pytest.mark.parametrize("path", ["closed", "numpy"])
def test_minimal_solver_on_the_reference_fixtures(name, path):
    x1, x2, E, tol = cases.fixture(name)
    args = _lists(x1, x2)
    h = model.five_point(*args, path=path)
    assert h.ok
    cosines = []
    for m in h.models:
        worst = max(model.sampson(m.F, args[0][k], args[1][k], args[2][k], args[3][k]) for k in range(5))
        assert worst < 1e-8, worst
        Em = np.array(m.F)
        cosines.append(abs(float((Em * E).sum())) / (np.linalg.norm(Em) * np.linalg.norm(E)))
    print(name, path, h.num_real_roots, len(h.models), 1.0 - max(cosines))
    assert max(cosines) >= 1.0 - tol  # test::ArraysEqualUpToScale


def test_ransac_recovers_the_pose_without_noise():
    b = synth.make_calibrated_pair_batch(4, 60, 3, inlier_ratio=1.0, pixel_noise=0.0)
    out = model.estimate(b["pair_offset"], b["feature1"], b["feature2"], cases.thresholds(b), seed=1, **cases.KW)
    assert (out["status"] == 0).all() and (out["num_inliers"] == 60).all()
    from scipy.spatial.transform import Rotation
    for p in range(4):
        loop = Rotation.from_rotvec(out["rotation"][p]) * Rotation.from_rotvec(b["rotation"][p]).inv()
        rot_deg = math.degrees(np.linalg.norm(loop.as_rotvec()))
        cosang = float(np.dot(out["position"][p], b["position"][p]) / np.linalg.norm(out["position"][p]))
        dir_deg = math.degrees(math.acos(min(1.0, cosang)))
        print(p, rot_deg, dir_deg)
        assert rot_deg < 1e-4 and dir_deg < 1e-4


def _host_check(tmp_path):
    exe = str(tmp_path / "two_view_calibrated_host_check")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    cmd = [entry._hipcc(), "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", *san,
           "-I" + os.path.join(ROOT, "theiasfm_amd", "csrc"), "-o", exe,
           os.path.join(ROOT, "tests", "cpp", "two_view_calibrated_host_check.cc")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr
    return exe


def test_the_kernels_text_on_the_host_gives_the_models_bits(tmp_path):
    """Every sample the main and planted models replayed, plus the reference's fixtures."""
    samples = []
    for b, m in ((cases.main_batch(), cases.main_model()), (cases.planted_batch(), cases.planted_model())):
        po, f1, f2 = b["pair_offset"], b["feature1"], b["feature2"]
        for p, r in m["results"].items():
            n = int(po[p + 1] - po[p])
            for i in sorted(r.hyp):
                s = b["samples"][p][i] if "samples" in b else model.sample(cases.MAIN_RANSAC_SEED, p, i, n)
                idx = po[p] + np.array(s, dtype=np.int64)
                samples.append(_lists(f1[idx], f2[idx]))
    for name in sorted(cases.FIXTURES):
        x1, x2, _, _ = cases.fixture(name)
        samples.append(_lists(x1, x2))
    text = "\n".join(" ".join(v.hex() for col in s for v in col) for s in samples) + "\n"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    p = subprocess.run([_host_check(tmp_path)], input=text, capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, p.stderr
    lines = p.stdout.split("\n")
    pos = 0
    for s in samples:
        h = model.five_point(*s)
        count = int(lines[pos])
        pos += 1
        assert count == len(h.models)
        for m in h.models:
            got = [float.fromhex(v).hex() for v in lines[pos].split()]
            pos += 1
            want = [float(v).hex() for v in [m.F[r][c] for r in range(3) for c in range(3)] + list(m.R) + list(m.p)]
            assert got == want
    assert len(samples) > 300


def test_argument_errors_come_before_the_device():
    b = cases.main_batch()
    po, f1, f2, th = b["pair_offset"], b["feature1"], b["feature2"], cases.thresholds(b)

    def status(**kw):
        args = dict(pair_offset=po, feature1=f1, feature2=f2, pair_error_threshold=th,
                    options=abi.two_view_ransac_options(**cases.KW))
        args.update(kw)
        try:
            lib.estimate_calibrated_relative_poses(**args)
        except lib.EngineError as e:
            return e.status
        return 0

    bad_po = po.copy()
    bad_po[3] = bad_po[2] - 1
    assert status(pair_offset=bad_po) == abi.ERR_INVALID_ARGUMENT
    bad_th = th.copy()
    bad_th[5] = 0.0
    assert status(pair_error_threshold=bad_th) == abi.ERR_INVALID_ARGUMENT
    for kw in (dict(failure_probability=0.0), dict(failure_probability=1.0), dict(min_inlier_ratio=1.5),
               dict(min_iterations=10, max_iterations=5), dict(max_iterations=(1 << 20) + 1),
               dict(chunk_iterations=-1)):
        assert status(options=abi.two_view_ransac_options(**kw)) == abi.ERR_INVALID_ARGUMENT, kw
    samples = np.zeros((len(cases.MAIN_COUNTS), cases.MAX_ITERATIONS, 5), np.int32)
    samples[:] = [0, 1, 2, 3, 4]
    samples[4, 7] = [0, 1, 2, 3, 3]  # a repeated index
    assert status(samples=samples) == abi.ERR_INVALID_ARGUMENT
    samples[4, 7] = [0, 1, 2, 3, 64]  # pair 4 has 64 correspondences
    assert status(samples=samples) == abi.ERR_INVALID_ARGUMENT
