"""The one compile line of the tests/test_host_shim_*.py wrappers: a program under tests/cpp and the host shim sources
it needs, g++ -Wall -Werror against the in-tree engine library, into pytest's tmp_path."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

LIB = os.path.join(ROOT, "theiasfm_amd", "lib")
HOST = os.path.join(ROOT, "theiasfm_amd", "host")


def compile_shim(tmp_path, test_source, shim_sources, extra_flags=()):
    """Builds the engine if it is stale, then tests/cpp/<test_source> with theiasfm_amd/host/<each of shim_sources>;
    extra_flags go after the common flags (so "-Wno-error" takes -Werror back).  Returns the executable."""
    entry.build_engine()
    exe = str(tmp_path / os.path.splitext(test_source)[0])
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-pthread", *extra_flags,
           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "cpp", test_source),
           *[os.path.join(HOST, source) for source in shim_sources],
           "-L" + LIB, "-ltheia_mi355_ba", "-Wl,-rpath," + LIB, "-Wl,-rpath,/opt/rocm/lib",
           "-Wl,-rpath-link,/opt/rocm/lib"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    return exe
