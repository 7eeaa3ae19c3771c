"""-m gpu: theia::TrackEstimator (theiasfm_amd/host/track_estimate_ops.cc) equals an in-test restatement of
EstimateTrack -- midpoint triangulation on PINHOLE without distortion, the shim's per-call BundleAdjustTrack, the
acceptance test -- track by track: the estimated set, IsEstimated, the points and the Summary fields, for
EstimateTracks and EstimateAllTracks (tests/cpp/test_track_estimator_shim.cc, compiled here with g++ into pytest's
tmp_path)."""
import os
import subprocess

import pytest

from shim_build import compile_shim


def _compile(tmp_path):
    # (this program is built with -Wall, without -Werror)
    return compile_shim(tmp_path, "test_track_estimator_shim.cc", ["bundle_adjuster.cc", "track_estimate_ops.cc"],
                        ("-Wno-error",))


def test_track_estimator_shim_compiles(tmp_path):
    assert os.path.exists(_compile(tmp_path))


@pytest.mark.gpu
def test_track_estimator_equals_restatement(tmp_path):
    exe = _compile(tmp_path)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
