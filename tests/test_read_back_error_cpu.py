"""Which error the finish of a one-shot call reports (ReadBack in theiasfm_amd/csrc/one_shot.h, the order factored
out into read_back_error.h), compiled for the host (tests/cpp/read_back_error_check.cc: its own main, under
-fsanitize=address,undefined): the last launch's before the copies' before the synchronise's, and success only if all
three succeeded -- all eight combinations of ok / failed."""
import itertools
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

STEPS = ("launch", "copy", "sync")


@pytest.fixture(scope="module")
def reported(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("read_back") / "read_back_error_check")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    cmd = [entry._hipcc(), "-x", "hip", "--cuda-host-only", "-O1", "-g", "-std=c++17", *san,
           "-I" + os.path.join(ROOT, "theiasfm_amd", "csrc"), "-o", exe,
           os.path.join(ROOT, "tests", "cpp", "read_back_error_check.cc")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    q = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert q.returncode == 0, q.stderr
    table = {}
    for line in q.stdout.splitlines():
        *state, answer = line.split()
        table[tuple(state)] = answer
    return table


def test_every_combination_is_answered(reported):
    assert len(reported) == 8


@pytest.mark.parametrize("failed", list(itertools.product((False, True), repeat=3)),
                         ids=lambda f: "+".join(s for s, x in zip(STEPS, f) if x) or "ok")
def test_launch_before_copy_before_sync(reported, failed):
    state = tuple(step if bad else "ok" for step, bad in zip(STEPS, failed))
    expected = next((step for step, bad in zip(STEPS, failed) if bad), "ok")
    assert reported[state] == expected
