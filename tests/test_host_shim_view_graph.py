"""theia::ViewGraph and the view-graph shim (theiasfm_amd/host/view_graph_ops.cc) through
tests/cpp/test_view_graph_shim.cc, compiled here with g++ -Wall -Werror into pytest's tmp_path.  Whatever the machine
has, the program checks the ViewGraph semantics of the reference's view_graph_test.cc; without a device that
RemoveDisconnectedViewPairs, OrientationsFromMaximumSpanningTree and the ViewGraph forms of the two filters change
nothing; with one (-m gpu) that they agree with the C ABI."""
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
    exe = str(tmp_path / "test_view_graph_shim")
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-pthread", "-I" + os.path.join(ROOT, "include"), "-o", exe,
           os.path.join(ROOT, "tests", "cpp", "test_view_graph_shim.cc"),
           os.path.join(ROOT, "theiasfm_amd", "host", "view_graph_ops.cc"),
           os.path.join(ROOT, "theiasfm_amd", "host", "view_pair_filter_ops.cc"),
           "-L" + LIB, "-ltheia_mi355_ba", "-Wl,-rpath," + LIB, "-Wl,-rpath,/opt/rocm/lib",
           "-Wl,-rpath-link,/opt/rocm/lib"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    return exe


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
