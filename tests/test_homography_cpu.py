"""The numpy model of tmi_ba_estimate_homographies (tests/homography_model.py) on its own, the sampler of four against
the host build of ransac_core.h, the flagging cap on exactly the inputs of tests/test_gpu_homography.py, the host-only
builders of the shim under the host sanitizers (a stand-alone program; nothing is loaded into python) and the call's
argument errors through the C ABI (which come before the device is looked for): no GPU needed.

Tolerances of the closed forms:
  recovery  four exact correspondences of a known H give H back up to scale within 1e-12 (the issue's bound: the
            normalised DLT of four well-spread points of size O(1) is conditioned far below 1e3, and 1e3 roundoffs are
            2e-13)
  transfer  H maps its four sample points onto their partners: a coordinate error below 1e-12 of O(1) coordinates, so a
            squared residual below 1e-24"""
import itertools
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
import homography_cases as cases  # noqa: E402
import homography_model as model  # noqa: E402
from shim_build import compile_shim  # noqa: E402
from theiasfm_amd import abi, lib  # noqa: E402


def _four(f1, f2, idx):
    return [[float(v) for v in a[idx, c]] for a, c in ((f1, 0), (f1, 1), (f2, 0), (f2, 1))]


@pytest.mark.parametrize("path", ["closed", "numpy"])
def test_exact_correspondences_give_the_homography_back(path):
    rng = np.random.default_rng(3)
    for _ in range(20):
        f1, f2, _, H = cases.plane_pair(rng, 12, 0.0, 0.0)
        h = model.hypothesis(*_four(f1, f2, np.array([0, 3, 6, 9])), path)
        assert h.ok
        got = model.unit_h(np.array(h.H).reshape(3, 3).T.reshape(9))[0]
        want = model.unit_h(H.T.reshape(9))[0]
        assert np.abs(got - want).max() < 1e-12
        # H maps the four sample points onto their partners, and every other point of the plane too
        r = model.residuals(h.H, f1[:, 0], f1[:, 1], f2[:, 0], f2[:, 1])
        assert r[[0, 3, 6, 9]].max() < 1e-24 and r.max() < 1e-20


def test_mle_cost_of_all_outliers_is_the_fixed_shape_sum_of_thresholds():
    b = cases.main_batch()
    for p in (3, 4, 5, 6):  # 63, 64, 65, 130 correspondences
        a, e = int(b["pair_offset"][p]), int(b["pair_offset"][p + 1])
        h = model.Hypothesis()
        h.H = [1.0, 0.0, 50.0, 0.0, 1.0, -50.0, 0.0, 0.0, 1.0]  # a shift far beyond every threshold
        inlier, mle, _ = model.score(h, b["feature1"][a:e, 0], b["feature1"][a:e, 1], b["feature2"][a:e, 0],
                                     b["feature2"][a:e, 1], cases.THRESHOLD)
        assert not inlier.any()
        assert mle == model.wave_sum(np.full(e - a, cases.THRESHOLD))
        assert abs(mle - (e - a) * cases.THRESHOLD) <= 64 * np.finfo(float).eps * mle
    # the shape itself: lane sums in ascending order, then the butterfly -- not np.sum's pairwise order
    v = np.random.default_rng(1).uniform(size=130)
    lanes = [0.0] * 64
    for q, x in enumerate(v):
        lanes[q % 64] = lanes[q % 64] + float(x)
    for off in (32, 16, 8, 4, 2, 1):
        lanes = [lanes[l] + lanes[l ^ off] for l in range(64)]
    assert model.wave_sum(v) == lanes[0] and len(set(lanes)) == 1


def test_the_two_model_paths_agree():
    """MODEL_SPREAD per input (DESIGN 8.20 records the values)."""
    for mle in (False, True):
        a, c = cases.main_model(mle), cases.main_model(mle, "numpy")
        spread = model.model_spread(a, c)
        print("MODEL_SPREAD use_mle", mle, spread)
        same = a["best_iteration"] == c["best_iteration"]
        assert np.array_equal(a["num_inliers"][same], c["num_inliers"][same])
        assert spread < 1e-9  # the margin below which a decision counts as open


def test_ransac_sample_of_four_matches_the_models_sampler(tmp_path):
    """ransac_sample<4> of theiasfm_amd/csrc/ransac_core.h, compiled for the host under -fsanitize=address,undefined
    (tests/cpp/ransac_sample4_host_check.cc: its own main), as tests/test_ransac_core_cpu.py does for 3, 5 and 8."""
    exe = str(tmp_path / "ransac_sample4_host_check")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    cmd = [entry._hipcc(), "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", *san,
           "-I" + os.path.join(ROOT, "theiasfm_amd", "csrc"), "-o", exe,
           os.path.join(ROOT, "tests", "cpp", "ransac_sample4_host_check.cc")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr
    inputs = [(seed, stream, i, n) for n in (4, 5, 8, 1000)
              for seed, stream, i in itertools.product((0, 0x9E3779B97F4A7C15), (0, 1, 2**32 - 1), (0, 1, 2**20 - 1))]
    text = "".join("%d %d %d %d\n" % c for c in inputs)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, p.stderr
    lines = p.stdout.splitlines()
    assert len(lines) == len(inputs)
    for (seed, stream, i, n), line in zip(inputs, lines):
        want = tuple(model.sample(seed, stream, i, n))
        assert tuple(map(int, line.split())) == want, (seed, stream, i, n)
        assert len(set(want)) == 4 and all(0 <= k < n for k in want)


def test_reference_scene():
    """estimate_homography_test.cc:127-128: EstimateHomography succeeds and more than 4 correspondences are inliers, in
    all four variants; without noise and outliers all 81 are."""
    o = cases.reference_model()
    assert (o["status"] == 0).all()
    assert (o["num_inliers"] > 4).all()
    assert (o["num_inliers"][:6] == 81).all()
    # (not the reference's assertion: the 70 % variants without noise find exactly the lattice's 57 inliers)
    assert (o["num_inliers"][12:18] == 57).all()


@pytest.mark.parametrize("name,use_mle", [("main", False), ("main", True), ("planted", False), ("planted", True),
                                          ("reference", True)])
def test_margins_on_the_gpu_tests_inputs(name, use_mle):
    """What tests/test_gpu_homography.py relies on: at most 2 % of the replayed hypotheses have a decision margin below
    1e-9 under either scoring, and none of those is the best model of its pair or changes its pair's bound."""
    if name == "reference":  # (the reference's scene is run with use_mle only)
        o = cases.reference_model()
    else:
        o = cases.main_model(use_mle) if name == "main" else cases.planted_model(use_mle)
    replayed = sum(len(r.hyp) for r in o["results"].values())
    flagged = sum(len(r.flagged) for r in o["results"].values())
    print(name, use_mle, "replayed", replayed, "flagged", flagged)
    assert replayed > 0 and flagged <= 0.02 * replayed
    for p, r in o["results"].items():
        assert r.best_iteration not in r.flagged, p
        assert not (r.flagged & r.bound_changers), p
    if name == "main":
        assert any(r.bound_changers for r in o["results"].values())  # the bound does drop somewhere
    if name == "planted":
        assert o["results"][0].hyp[0].reason == "rank" and o["results"][0].hyp[0].min_margin() >= model.MARGIN
        assert o["results"][1].hyp[0].reason == "rank"
        assert o["status"][2] == 2 and o["num_iterations"][2] == cases.MAX_ITERATIONS


def test_the_two_scorings_differ_somewhere():
    """tests/test_gpu_homography.py uses cases.MLE_PAIR to show that the MLE path is taken on the device."""
    a, c = cases.main_model(False), cases.main_model(True)
    assert a["best_iteration"][cases.MLE_PAIR] != c["best_iteration"][cases.MLE_PAIR]
    r = c["results"][cases.MLE_PAIR]
    assert r.best_iteration not in r.flagged
    # under MLE the integer of a hypothesis is still n - inliers: the two runs agree on it wherever both replayed it
    both = (a["hypothesis_cost"] >= 0) & (c["hypothesis_cost"] >= 0)
    assert np.array_equal(a["hypothesis_cost"][both], c["hypothesis_cost"][both])


def _reference_loop(costs, inliers, n, failure_probability, min_iterations, max_iterations):
    """sample_consensus_estimator.h:276-330 over precomputed costs (None: EstimateModel returned false)."""
    log_fp = math.log(failure_probability)
    best_cost, best_it, bound, it = float("inf"), -1, max_iterations, 0
    while it < bound:
        c = costs[it]
        it += 1
        if c is None:
            continue
        if c < best_cost:
            best_cost, best_it = c, it - 1
            ratio = inliers[it - 1] / n
            if ratio < 4 / n:
                continue
            bound = min(model.compute_max_iterations(ratio, log_fp, min_iterations, max_iterations), bound)
    return it, best_it


@pytest.mark.parametrize("use_mle", [False, True])
def test_replay_against_the_reference_loop(use_mle):
    for o in (cases.main_model(use_mle), cases.main_model(use_mle, "closed", 5), cases.planted_model(use_mle)):
        for p, r in o["results"].items():
            ok = [i in r.hyp and r.hyp[i].ok for i in range(cases.MAX_ITERATIONS)]
            costs = [(r.hyp[i].cost_real if use_mle else r.hyp[i].cost) if ok[i] else None
                     for i in range(cases.MAX_ITERATIONS)]
            inliers = [r.hyp[i].inliers if ok[i] else 0 for i in range(cases.MAX_ITERATIONS)]
            assert _reference_loop(costs, inliers, r.n, 0.01, cases.MIN_ITERATIONS, cases.MAX_ITERATIONS) == \
                (r.num_iterations, r.best_iteration), p
    a, c = cases.main_model(use_mle), cases.main_model(use_mle, "closed", 5)
    for k in ("status", "num_inliers", "num_iterations", "best_iteration", "hypothesis_cost", "corr_inlier"):
        assert np.array_equal(a[k], c[k]), k
    assert a["hypothesis_cost_real"].tobytes() == c["hypothesis_cost_real"].tobytes()
    assert model.compute_max_iterations(1.0, math.log(0.01), 16, 64) == 16
    assert model.compute_max_iterations(0.5, math.log(0.01), 10, 5000) == 71  # log(0.01) / log(1 - 2^-4)


def test_host_builders_under_host_sanitizers(tmp_path):
    """The shim's host-only builders (the threshold of CountHomographyInliers and the option mapping) in a stand-alone
    program with -fsanitize=address,undefined (tests/cpp/homography_builders_host_check.cc; the engine library is not
    instrumented and no device is touched)."""
    exe = compile_shim(tmp_path, "homography_builders_host_check.cc",
                       ["homography_ops.cc", "localize_ops.cc", "view_ops.cc", "bundle_adjuster.cc"],
                       ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    print(p.stdout, p.stderr)
    assert p.returncode == 0 and "homography builders: OK" in p.stdout, p.stdout + p.stderr


def test_argument_errors():
    """Returned before the device is looked for, so they need none."""
    b = cases.planted_batch()
    po, f1, f2, sm = b["pair_offset"], b["feature1"], b["feature2"], b["samples"]
    th = np.full(3, cases.THRESHOLD)

    def status(**kw):
        args = dict(pair_offset=po, feature1=f1, feature2=f2, pair_error_threshold=th,
                    options=abi.homography_ransac_options(**cases.KW))
        args.update(kw)
        with pytest.raises(lib.EngineError) as e:
            lib.estimate_homographies(**args)
        return e.value.status

    bad = sm.copy()
    bad[1, 7, 0] = bad[1, 7, 3]
    assert status(samples=bad) == abi.ERR_INVALID_ARGUMENT
    bad = sm.copy()
    bad[2, 0, 3] = 6
    assert status(samples=bad) == abi.ERR_INVALID_ARGUMENT
    assert status(pair_error_threshold=np.array([4e-6, 0.0, 4e-6])) == abi.ERR_INVALID_ARGUMENT
    assert status(pair_error_threshold=np.array([4e-6, np.nan, 4e-6])) == abi.ERR_INVALID_ARGUMENT
    assert status(pair_offset=np.array([0, 40, 30, 86])) == abi.ERR_INVALID_ARGUMENT
    assert status(pair_offset=np.array([1, 40, 80, 86])) == abi.ERR_INVALID_ARGUMENT
    for kw in (dict(failure_probability=0.0), dict(failure_probability=1.0), dict(min_inlier_ratio=1.5),
               dict(min_iterations=65, max_iterations=64), dict(max_iterations=(1 << 20) + 1),
               dict(chunk_iterations=-1)):
        for mle in (0, 1):
            assert status(options=abi.homography_ransac_options(use_mle=mle, **kw)) == abi.ERR_INVALID_ARGUMENT, kw
    # the real costs exist under MLE only
    assert status(want_hypothesis_cost_real=True) == abi.ERR_INVALID_ARGUMENT
    # a bad sample of a pair that is NOT attempted (masked out) is not looked at: the call gets as far as the device
    bad = sm.copy()
    bad[1, 7, 0] = bad[1, 7, 3]
    for mle in (0, 1):
        try:
            lib.estimate_homographies(po, f1, f2, th, options=abi.homography_ransac_options(use_mle=mle, **cases.KW),
                                      pair_mask=[1, 0, 1], samples=bad, want_hypothesis_cost_real=bool(mle))
        except lib.EngineError as e:
            assert e.status != abi.ERR_INVALID_ARGUMENT
    o = abi.homography_ransac_options()
    L = lib.load()
    c = abi.CHomographyRansacOptions()
    c.use_mle = 7
    L.tmi_ba_homography_ransac_options_init(c)
    for name, _ in abi.CHomographyRansacOptions._fields_:
        assert getattr(o, name) == getattr(c, name), name
    assert (c.min_iterations, c.max_iterations, c.failure_probability, c.use_mle) == (10, 1000, 0.01, 0)
    # the sibling calls' options keep their layout: the new struct only appends to it
    assert abi.CHomographyRansacOptions._fields_[:7] == abi.CTwoViewRansacOptions._fields_
