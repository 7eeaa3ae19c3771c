"""-m gpu: the two-view verification shim (theiasfm_amd/host/two_view_verify_ops.cc) through
tests/cpp/test_two_view_verification_shim.cc, compiled here with g++ into pytest's tmp_path: the single call equals the
batch call equals the C ABI bit for bit, position_2 has unit norm, inlier_indices are the status-0 indices in order."""
import os
import subprocess

import pytest

from shim_build import compile_shim


def _compile(tmp_path):
    return compile_shim(tmp_path, "test_two_view_verification_shim.cc", ["two_view_verify_ops.cc"])


def test_two_view_verification_shim_test_compiles(tmp_path):
    assert os.path.exists(_compile(tmp_path))


@pytest.mark.gpu
def test_two_view_verification_shim_equals_abi(tmp_path):
    exe = _compile(tmp_path)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
