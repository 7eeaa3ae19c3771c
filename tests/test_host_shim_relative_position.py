"""-m gpu: the relative-position shim (theiasfm_amd/host/relative_position_ops.cc) through
tests/cpp/test_relative_position_shim.cc, compiled here with g++ into pytest's tmp_path: the single call equals the
batch call equals the C ABI bit for bit, and RefineRelativeTranslationsWithKnownRotations on a small Reconstruction
equals an in-test restatement that normalises the pixels on the host."""
import os
import subprocess

import pytest

from shim_build import compile_shim


def _compile(tmp_path):
    # (this program is built with -Wall, without -Werror)
    return compile_shim(tmp_path, "test_relative_position_shim.cc", ["bundle_adjuster.cc", "relative_position_ops.cc"],
                        ("-Wno-error",))


def test_relative_position_shim_test_compiles(tmp_path):
    assert os.path.exists(_compile(tmp_path))


@pytest.mark.gpu
def test_relative_position_shim_equals_abi_and_restatement(tmp_path):
    exe = _compile(tmp_path)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
