"""The homography shim (theiasfm_amd/host/homography_ops.cc) through tests/cpp/test_homography_shim.cc, compiled here
with g++ -Wall -Werror into pytest's tmp_path: the signature and defaults against the reference's, the refusals with the
outputs untouched and, without a device, false with the outputs untouched; with one (-m gpu) EstimateHomography on the
reference's lattice scene, CountHomographyInliers equal to the C ABI call's count for the same threshold and the batched
form writing TwoViewInfo::num_homography_inliers.  The same program also runs as a stand-alone binary under the host's
address and undefined-behaviour sanitizers (its own main; nothing is loaded into python)."""
import os
import subprocess

import pytest

from shim_build import compile_shim

NO_DEVICE = dict(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")


def _compile(tmp_path, extra=()):
    return compile_shim(tmp_path, "test_homography_shim.cc",
                        ["homography_ops.cc", "localize_ops.cc", "view_ops.cc", "bundle_adjuster.cc"], extra)


def test_homography_shim_without_a_device(tmp_path):
    p = subprocess.run([_compile(tmp_path)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, **NO_DEVICE))
    print(p.stdout, p.stderr)
    assert p.returncode == 0 and "homography shim: OK" in p.stdout, p.stdout + p.stderr


def test_homography_shim_under_host_sanitizers(tmp_path):
    """The stand-alone program with -fsanitize=address,undefined on the shim and the test (the engine library is not
    instrumented).  Leak checking is off: the HIP runtime's start-up allocations are not the shim's."""
    exe = _compile(tmp_path,
                   ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", **NO_DEVICE)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    print(p.stdout, p.stderr)
    assert p.returncode == 0 and "homography shim: OK" in p.stdout, p.stdout + p.stderr


@pytest.mark.gpu
def test_homography_shim_on_the_device(tmp_path):
    p = subprocess.run([_compile(tmp_path), "--need-device"], capture_output=True, text=True, timeout=600)
    print(p.stdout, p.stderr)
    assert p.returncode == 0 and "homography shim: OK (device)" in p.stdout, p.stdout + p.stderr
