"""The one sampler of the batched RANSAC calls (theiasfm_amd/csrc/ransac_core.h), compiled for the host (its own main,
under -fsanitize=address,undefined), against the sample function of each call's independent numpy model: a sample of
three (localisation), five (calibrated pairs) and eight (uncalibrated pairs), at the sizes where the swaps collide and
the clamp bites."""
import itertools
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402
import localization_model  # noqa: E402
import two_view_calibrated_model  # noqa: E402
import two_view_ransac_model  # noqa: E402

MODELS = {3: localization_model.sample, 5: two_view_calibrated_model.sample, 8: two_view_ransac_model.sample}
SEEDS = (0, 0x9E3779B97F4A7C15)
STREAMS = (0, 1, 2**32 - 1)
ITERATIONS = (0, 1, 2**20 - 1)


def _host_check(tmp_path):
    exe = str(tmp_path / "ransac_sample_host_check")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    cmd = [entry._hipcc(), "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", *san,
           "-I" + os.path.join(ROOT, "theiasfm_amd", "csrc"), "-o", exe,
           os.path.join(ROOT, "tests", "cpp", "ransac_sample_host_check.cc")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr
    return exe


def test_the_shared_sampler_gives_each_models_samples(tmp_path):
    cases = [(N, seed, stream, i, n) for N in MODELS for n in (N, N + 1, 2 * N, 1000)
             for seed, stream, i in itertools.product(SEEDS, STREAMS, ITERATIONS)]
    assert len(cases) == 3 * 4 * 2 * 3 * 3
    text = "".join("%d %d %d %d %d\n" % c for c in cases)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    p = subprocess.run([_host_check(tmp_path)], input=text, capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, p.stderr
    lines = p.stdout.splitlines()
    assert len(lines) == len(cases)
    for (N, seed, stream, i, n), line in zip(cases, lines):
        want = tuple(MODELS[N](seed, stream, i, n))
        assert tuple(map(int, line.split())) == want, (N, seed, stream, i, n)
        assert len(set(want)) == N and all(0 <= k < n for k in want)
