"""-m gpu: the two-view verification shim (theiasfm_amd/host/two_view_verify_ops.cc) through
tests/cpp/test_two_view_verification_shim.cc, compiled here with g++ into pytest's tmp_path: the single call equals the
batch call equals the C ABI bit for bit, position_2 has unit norm, inlier_indices are the status-0 indices in order."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

LIB = os.path.join(ROOT, "theiasfm_amd", "lib")


def _compile(tmp_path):
    entry.build_engine()
    exe = str(tmp_path / "test_two_view_verification_shim")
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-pthread", "-I" + os.path.join(ROOT, "include"), "-o", exe,
           os.path.join(ROOT, "tests", "cpp", "test_two_view_verification_shim.cc"),
           os.path.join(ROOT, "theiasfm_amd", "host", "two_view_verify_ops.cc"),
           "-L" + LIB, "-ltheia_mi355_ba", "-Wl,-rpath," + LIB, "-Wl,-rpath,/opt/rocm/lib",
           "-Wl,-rpath-link,/opt/rocm/lib"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    return exe


def test_two_view_verification_shim_test_compiles(tmp_path):
    assert os.path.exists(_compile(tmp_path))


@pytest.mark.gpu
def test_two_view_verification_shim_equals_abi(tmp_path):
    exe = _compile(tmp_path)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
