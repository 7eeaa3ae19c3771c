"""CPU-side checks of the batched BundleAdjustView boundary (tmi_ba_adjust_views / tmi_ba_solver_adjust_views):
both symbols are exported and argument errors are reported before any device work."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402
from theiasfm_amd import abi, lib, synth  # noqa: E402

INVALID_ARGUMENT = 1


@pytest.fixture(scope="module")
def L():
    entry.build_engine()
    return lib.load()


def test_symbols_exported(L):
    for name in ("tmi_ba_adjust_views", "tmi_ba_solver_adjust_views"):
        assert name in lib.EXPORTS
        assert hasattr(L, name)


def test_null_arguments_are_invalid(L):
    P = synth.make_problem(4, 50, 200, seed=0)
    cp = P.as_c()
    o = abi.default_options()
    s = abi.CViewBatchSummary()
    assert L.tmi_ba_adjust_views(None, C.byref(o), None, None, None, None, None, C.byref(s)) == INVALID_ARGUMENT
    assert L.tmi_ba_adjust_views(C.byref(cp), None, None, None, None, None, None, C.byref(s)) == INVALID_ARGUMENT
    assert L.tmi_ba_adjust_views(C.byref(cp), C.byref(o), None, None, None, None, None, None) == INVALID_ARGUMENT
    assert L.tmi_ba_solver_adjust_views(None, C.byref(o), None, None, None, None, None, C.byref(s)) == INVALID_ARGUMENT


def test_bad_observation_index_is_invalid(L):
    P = synth.make_problem(4, 50, 200, seed=0)
    P.obs_camera[3] = P.num_cameras  # out of range: refused before the device is touched
    o = abi.default_options()
    with pytest.raises(lib.EngineError) as e:
        lib.adjust_views(P, o)
    assert e.value.status == INVALID_ARGUMENT


def test_summary_layout():
    assert C.sizeof(abi.CViewBatchSummary) == 48
    assert abi.CViewBatchSummary.kernel_seconds.offset == 40
