"""The position estimator shim (theiasfm_amd/host/position_ops.cc) through tests/cpp/test_position_estimator_shim.cc,
compiled here with g++ -Wall -Werror into pytest's tmp_path.  Without a device the program checks that the call returns
false and leaves the position map unchanged; with one (-m gpu) it checks the id mapping in ascending order, the dropped
pairs and the error paths against the C ABI called directly."""
import subprocess

import pytest

from shim_build import compile_shim


def _compile(tmp_path):
    return compile_shim(tmp_path, "test_position_estimator_shim.cc", ["position_ops.cc"])


def test_position_estimator_shim(tmp_path):
    """Whatever the machine has: without a device false and an unchanged map, with one the full comparison."""
    p = subprocess.run([_compile(tmp_path)], capture_output=True, text=True, timeout=600)
    print(p.stdout, p.stderr)
    assert p.returncode == 0 and "OK" in p.stdout, p.stdout + p.stderr


@pytest.mark.gpu
def test_position_estimator_shim_on_the_device(tmp_path):
    p = subprocess.run([_compile(tmp_path), "--need-device"], capture_output=True, text=True, timeout=600)
    print(p.stdout, p.stderr)
    assert p.returncode == 0 and "position estimator shim: OK" in p.stdout, p.stdout + p.stderr
