"""The track builder shim (theiasfm_amd/host/track_builder_ops.cc) through tests/cpp/test_track_builder_shim.cc,
compiled here with g++ -Wall -Werror into pytest's tmp_path: the defaults and, without a device, BuildTracks returning
false with the reconstruction's tracks unchanged; with one (-m gpu) the reference's five tests with its VerifyTracks,
bulk add == single adds and an unknown view.  The same program also runs as a stand-alone binary under the host's
address and undefined-behaviour sanitizers (its own main; nothing is loaded into python)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

LIB = os.path.join(ROOT, "theiasfm_amd", "lib")
HOST = os.path.join(ROOT, "theiasfm_amd", "host")
NO_DEVICE = dict(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")


def _compile(tmp_path, name="test_track_builder_shim", extra=()):
    entry.build_engine()
    exe = str(tmp_path / name)
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-pthread", *extra, "-I" + os.path.join(ROOT, "include"),
           "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_track_builder_shim.cc"),
           os.path.join(HOST, "track_builder_ops.cc"),
           "-L" + LIB, "-ltheia_mi355_ba", "-Wl,-rpath," + LIB, "-Wl,-rpath,/opt/rocm/lib",
           "-Wl,-rpath-link,/opt/rocm/lib"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    return exe


def test_track_builder_shim_without_a_device(tmp_path):
    p = subprocess.run([_compile(tmp_path)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, **NO_DEVICE))
    print(p.stdout, p.stderr)
    assert p.returncode == 0 and "track builder shim: OK" in p.stdout, p.stdout + p.stderr


def test_track_builder_shim_under_host_sanitizers(tmp_path):
    """The stand-alone program with -fsanitize=address,undefined on the shim and the test (the engine library is not
    instrumented), no device visible.  Leak checking is off: the HIP runtime's start-up allocations are not the
    shim's."""
    exe = _compile(tmp_path, "test_track_builder_shim_san",
                   ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", **NO_DEVICE)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    print(p.stdout, p.stderr)
    assert p.returncode == 0 and "track builder shim: OK" in p.stdout, p.stdout + p.stderr


@pytest.mark.gpu
def test_track_builder_shim_on_the_device(tmp_path):
    p = subprocess.run([_compile(tmp_path), "--need-device"], capture_output=True, text=True, timeout=600)
    print(p.stdout, p.stderr)
    assert p.returncode == 0 and "track builder shim: OK (device)" in p.stdout, p.stdout + p.stderr
