"""The matching shim (theiasfm_amd/host/match_ops.cc) through tests/cpp/test_matching_shim.cc, compiled here with
g++ -Wall -Werror into pytest's tmp_path: the defaults against the reference's and, without a device, false and empty
outputs; with one (-m gpu) the reference's three tests through the shim, batch == single calls and the correspondence
helper.  The same program also runs as a stand-alone binary under the host's address and undefined-behaviour
sanitizers (its own main; nothing is loaded into python)."""
import os
import subprocess

import pytest

from shim_build import compile_shim

NO_DEVICE = dict(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")


def _compile(tmp_path, extra=()):
    return compile_shim(tmp_path, "test_matching_shim.cc", ["match_ops.cc"], extra)


def test_matching_shim_without_a_device(tmp_path):
    p = subprocess.run([_compile(tmp_path)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, **NO_DEVICE))
    print(p.stdout, p.stderr)
    assert p.returncode == 0 and "matching shim: OK" in p.stdout, p.stdout + p.stderr


def test_matching_shim_under_host_sanitizers(tmp_path):
    """The stand-alone program with -fsanitize=address,undefined on the shim and the test (the engine library is not
    instrumented), no device visible.  Leak checking is off: the HIP runtime's start-up allocations are not the
    shim's."""
    exe = _compile(tmp_path,
                   ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", **NO_DEVICE)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    print(p.stdout, p.stderr)
    assert p.returncode == 0 and "matching shim: OK" in p.stdout, p.stdout + p.stderr


@pytest.mark.gpu
def test_matching_shim_on_the_device(tmp_path):
    p = subprocess.run([_compile(tmp_path), "--need-device"], capture_output=True, text=True, timeout=600)
    print(p.stdout, p.stderr)
    assert p.returncode == 0 and "matching shim: OK (device)" in p.stdout, p.stdout + p.stderr
