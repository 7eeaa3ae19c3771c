"""The nonlinear rotation estimator shim (theiasfm_amd/host/nonlinear_rotation_ops.cc) through
tests/cpp/test_nonlinear_rotation_estimator_shim.cc, compiled here with g++ -Wall -Werror into pytest's tmp_path.  The
program checks the defaults against the reference's and the two refusals (false, nothing written) on any machine; without
a device that the call returns false and leaves the map unchanged; with one (-m gpu) a 12-view noisy graph in which one
view is absent from the map -- it stays absent, the others change -- against the C ABI called directly on the same
flattened input, bit for bit."""
import subprocess

import pytest

from shim_build import compile_shim


def _compile(tmp_path):
    return compile_shim(tmp_path, "test_nonlinear_rotation_estimator_shim.cc", ["nonlinear_rotation_ops.cc"])


def test_nonlinear_rotation_estimator_shim(tmp_path):
    """Whatever the machine has: without a device false and an unchanged map, with one the full comparison."""
    p = subprocess.run([_compile(tmp_path)], capture_output=True, text=True, timeout=600)
    print(p.stdout, p.stderr)
    assert p.returncode == 0 and "OK" in p.stdout, p.stdout + p.stderr


@pytest.mark.gpu
def test_nonlinear_rotation_estimator_shim_on_the_device(tmp_path):
    p = subprocess.run([_compile(tmp_path), "--need-device"], capture_output=True, text=True, timeout=600)
    print(p.stdout, p.stderr)
    assert p.returncode == 0 and "nonlinear rotation estimator shim: OK" in p.stdout, p.stdout + p.stderr
