"""theia::ViewGraph and the view-graph shim (theiasfm_amd/host/view_graph_ops.cc) through
tests/cpp/test_view_graph_shim.cc, compiled here with g++ -Wall -Werror into pytest's tmp_path.  Whatever the machine
has, the program checks the ViewGraph semantics of the reference's view_graph_test.cc; without a device that
RemoveDisconnectedViewPairs, OrientationsFromMaximumSpanningTree and the ViewGraph forms of the two filters change
nothing; with one (-m gpu) that they agree with the C ABI."""
import subprocess

import pytest

from shim_build import compile_shim


def _compile(tmp_path):
    return compile_shim(tmp_path, "test_view_graph_shim.cc", ["view_graph_ops.cc", "view_pair_filter_ops.cc"])


def test_view_graph_shim(tmp_path):
    """Whatever the machine has: the ViewGraph semantics; without a device a clean refusal, with one the comparison."""
    p = subprocess.run([_compile(tmp_path)], capture_output=True, text=True, timeout=600)
    print(p.stdout, p.stderr)
    assert p.returncode == 0 and "OK" in p.stdout, p.stdout + p.stderr


@pytest.mark.gpu
def test_view_graph_shim_on_the_device(tmp_path):
    p = subprocess.run([_compile(tmp_path), "--need-device"], capture_output=True, text=True, timeout=600)
    print(p.stdout, p.stderr)
    assert p.returncode == 0 and "view-graph shim: OK" in p.stdout, p.stdout + p.stderr
