"""What the seven view-graph host shims hand to the C ABI and write back, byte for byte: tests/cpp/view_graph_shim_record.cc
links the shims with stand-ins for the entry points they call (not the engine), prints every batch, option struct and
input array it is given and every map, edge list and return value the caller gets back -- once with every device call
succeeding and once, with --fail, with every one failing -- and the two outputs together must equal
tests/golden/view_graph_shim_batches.txt, recorded from the shims as they were before theiasfm_amd/host/flat_view_graph.h
existed.  A shim that changes what it sends on purpose re-records the file and says so."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "theiasfm_amd", "host")
SHIMS = ["rotation_ops.cc", "nonlinear_rotation_ops.cc", "linear_rotation_ops.cc", "position_ops.cc",
         "nonlinear_position_ops.cc", "view_graph_ops.cc", "view_pair_filter_ops.cc"]


def test_view_graph_shims_send_and_write_back_what_they_did(tmp_path, golden_dir):
    exe = str(tmp_path / "view_graph_shim_record")
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
           os.path.join(ROOT, "tests", "cpp", "view_graph_shim_record.cc"), *[os.path.join(HOST, s) for s in SHIMS]]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    out = b""
    for args in ([], ["--fail"]):
        p = subprocess.run([exe, *args], capture_output=True, timeout=60)
        assert p.returncode == 0, p.stdout.decode() + p.stderr.decode()
        out += p.stdout
    with open(os.path.join(golden_dir, "view_graph_shim_batches.txt"), "rb") as f:
        want = f.read()
    if out != want:  # name the first line that differs; the whole output is a hundred kilobytes
        got_lines, want_lines = out.decode().splitlines(), want.decode().splitlines()
        for i, (g, w) in enumerate(zip(got_lines, want_lines)):
            assert g == w, f"line {i + 1}: got {g!r}, recorded {w!r}"
        assert len(got_lines) == len(want_lines), f"{len(got_lines)} lines, recorded {len(want_lines)}"
    assert out == want
