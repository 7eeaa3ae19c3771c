"""The view-pair filter shim (theiasfm_amd/host/view_pair_filter_ops.cc) through
tests/cpp/test_view_pair_filter_shim.cc, compiled here with g++ -Wall -Werror into pytest's tmp_path.  Without a
device the program checks that both calls leave the edge vector unchanged and return 0; with one (-m gpu) it checks
the id mapping in ascending order, the missing-orientation rule and the erasure against the C ABI."""
import subprocess

import pytest

from shim_build import compile_shim


def _compile(tmp_path):
    return compile_shim(tmp_path, "test_view_pair_filter_shim.cc", ["view_pair_filter_ops.cc"])


def test_view_pair_filter_shim(tmp_path):
    """Whatever the machine has: without a device no change and a return of 0, with one the full comparison."""
    p = subprocess.run([_compile(tmp_path)], capture_output=True, text=True, timeout=600)
    print(p.stdout, p.stderr)
    assert p.returncode == 0 and "OK" in p.stdout, p.stdout + p.stderr


@pytest.mark.gpu
def test_view_pair_filter_shim_on_the_device(tmp_path):
    p = subprocess.run([_compile(tmp_path), "--need-device"], capture_output=True, text=True, timeout=600)
    print(p.stdout, p.stderr)
    assert p.returncode == 0 and "view-pair filter shim: OK" in p.stdout, p.stdout + p.stderr
