"""The linear position estimator shim (theiasfm_amd/host/linear_position_ops.cc) through
tests/cpp/test_linear_position_estimator_shim.cc, compiled here with g++ -Wall -Werror into pytest's tmp_path.  The
program checks the defaults and the refusals (false, nothing written) on any machine, and this wrapper reads the refusal
messages from stderr; without a device that the call returns false and leaves the map unchanged; with one (-m gpu) the
reference's two tests on a theia::Reconstruction with scattered view ids, the key set of the result, and a graph without
a triangle."""
import subprocess

import pytest

from shim_build import compile_shim

TAG = "[theia::LinearPositionEstimator]"
MESSAGES = [
    "null positions",
    "number of view pairs = 0, number of orientations = ",
    ", number of orientations = 0",
    "num_threads, max_power_iterations and eigensolver_threshold must be positive",
    "the first id is not below the second",
    "no view pair between oriented views of the reconstruction",
]


def _compile(tmp_path):
    return compile_shim(tmp_path, "test_linear_position_estimator_shim.cc", ["linear_position_ops.cc"])


def _check_messages(stderr, more=()):
    for message in list(MESSAGES) + list(more):
        assert any(line.startswith(TAG) and message in line for line in stderr.splitlines()), message


def test_linear_position_estimator_shim(tmp_path):
    """Whatever the machine has: without a device false and an unchanged map, with one the full comparison."""
    p = subprocess.run([_compile(tmp_path)], capture_output=True, text=True, timeout=600)
    print(p.stdout, p.stderr)
    assert p.returncode == 0 and "OK" in p.stdout, p.stdout + p.stderr
    _check_messages(p.stderr)


@pytest.mark.gpu
def test_linear_position_estimator_shim_on_the_device(tmp_path):
    p = subprocess.run([_compile(tmp_path), "--need-device"], capture_output=True, text=True, timeout=600)
    print(p.stdout, p.stderr)
    assert p.returncode == 0 and "linear position estimator shim: OK" in p.stdout, p.stdout + p.stderr
    _check_messages(p.stderr, ["0 triplets, 0 with a baseline"])
