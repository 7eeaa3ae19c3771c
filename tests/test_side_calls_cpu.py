"""Argument checks of the batched two-view calls without a GPU: every bad input of tmi_ba_adjust_two_views and
tmi_ba_adjust_two_views_angular is TMI_BA_ERR_INVALID_ARGUMENT (1) before the device is looked for, a valid batch is
TMI_BA_ERR_NO_DEVICE (2) where there is none, and tmi_ba_adjust_two_views and tmi_ba_verify_two_views, which take the
same batch, give the same status for the same bad batch."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402
from theiasfm_amd import abi, lib, synth  # noqa: E402

INVALID_ARGUMENT, NO_DEVICE = 1, 2


@pytest.fixture(scope="module")
def L():
    entry.build_engine()
    return lib.load()


def _null(cb, name):
    setattr(cb, name, C.cast(None, type(getattr(cb, name))))


def _two_view(n_pairs=3):
    B, _ = synth.make_two_view_verification_batch(n_pairs, 5, roles=False, min_corr=35, max_corr=40)
    return B


def _angular(n_pairs=3):
    return synth.make_two_view_angular_batch(n_pairs, 5, min_corr=35, max_corr=40)[0]


def _adjust(L, cb, point_dof=4, iters=200, summary=True):
    s = abi.CTrackBatchSummary()
    return L.tmi_ba_adjust_two_views(None if cb is None else C.byref(cb), point_dof, iters, -1, None, None, None, None,
                                     C.byref(s) if summary else None)


def _adjust_angular(L, cb, iters=200, summary=True):
    s = abi.CTrackBatchSummary()
    return L.tmi_ba_adjust_two_views_angular(None if cb is None else C.byref(cb), iters, -1, None, None, None, None,
                                             C.byref(s) if summary else None)


def _verify(L, cb, point_dof=4, iters=200, summary=True):
    s = abi.CTwoViewVerificationSummary()
    o = abi.two_view_verification_options()
    return L.tmi_ba_verify_two_views(None if cb is None else C.byref(cb), C.byref(o), point_dof, iters, -1, None, None,
                                     None, None, None, None, None, C.byref(s) if summary else None)


# ---- the bad two-view batches: (name, batch -> (C batch or None, keyword arguments of the call)) -------------------
def _decreasing(B):
    B.correspondence_ptr[1] = B.correspondence_ptr[2] + 1
    return B.as_c(), {}


def _model(field):
    def make(B):
        getattr(B, field)[1] = 5
        return B.as_c(), {}
    return make


def _negative_pairs(B):
    cb = B.as_c()
    cb.num_pairs = -1
    return cb, {}


def _missing(field):
    def make(B):
        cb = B.as_c()
        _null(cb, field)
        return cb, {}
    return make


COMMON_ROWS = [
    ("null batch", lambda B: (None, {})),
    ("null summary", lambda B: (B.as_c(), {"summary": False})),
    ("negative pair count", _negative_pairs),
    ("negative iteration limit", lambda B: (B.as_c(), {"iters": -1})),
    ("decreasing correspondence_ptr", _decreasing),
]
TWO_VIEW_ROWS = COMMON_ROWS + [
    ("point_dof 2", lambda B: (B.as_c(), {"point_dof": 2})),
    ("model1 5", _model("model1")),
    ("model2 5", _model("model2")),
] + [("missing " + f, _missing(f)) for f in (
    "features1", "features2", "points",  # N > 0
    "extrinsics1", "extrinsics2", "model1", "model2", "intrinsics1", "intrinsics2", "correspondence_ptr")]
ANGULAR_ROWS = COMMON_ROWS + [("missing " + f, _missing(f)) for f in (
    "features1", "features2",  # N > 0
    "rotation2", "position2", "correspondence_ptr")]


@pytest.mark.parametrize("name,make", TWO_VIEW_ROWS, ids=[r[0] for r in TWO_VIEW_ROWS])
def test_adjust_two_views_rejects_before_the_device(L, name, make):
    B = _two_view()  # (kept alive: the C batch points into it)
    cb, kw = make(B)
    assert _adjust(L, cb, **kw) == INVALID_ARGUMENT


@pytest.mark.parametrize("name,make", ANGULAR_ROWS, ids=[r[0] for r in ANGULAR_ROWS])
def test_adjust_two_views_angular_rejects_before_the_device(L, name, make):
    B = _angular()
    cb, kw = make(B)
    assert _adjust_angular(L, cb, **kw) == INVALID_ARGUMENT


@pytest.mark.parametrize("name,make", TWO_VIEW_ROWS, ids=[r[0] for r in TWO_VIEW_ROWS])
def test_adjust_and_verify_agree_on_a_bad_batch(L, name, make):
    A, V = _two_view(), _two_view()
    ca, kw = make(A)
    cv, _ = make(V)
    assert _adjust(L, ca, **kw) == _verify(L, cv, **kw) == INVALID_ARGUMENT


def test_a_valid_pair_without_a_device_is_no_device(L):
    if L.tmi_ba_device_count() > 0:
        pytest.skip("a GPU is visible")
    B, G = _two_view(1), _angular(1)
    before, before_g = B.copy(), G.copy()
    assert _adjust(L, B.as_c()) == NO_DEVICE
    assert _adjust(L, B.as_c(), point_dof=3) == NO_DEVICE
    assert _adjust_angular(L, G.as_c()) == NO_DEVICE
    assert _verify(L, B.as_c()) == NO_DEVICE
    # absent constant_intrinsics mean "constant": not an argument error
    cb = B.as_c()
    _null(cb, "constant_intrinsics1")
    _null(cb, "constant_intrinsics2")
    assert _adjust(L, cb) == NO_DEVICE
    # an empty batch is looked at only after the device
    E = _two_view(1).head(0)
    assert _adjust(L, E.as_c()) == NO_DEVICE
    assert _adjust_angular(L, _angular(1).head(0).as_c()) == NO_DEVICE
    np.testing.assert_array_equal(B.extrinsics2, before.extrinsics2)
    np.testing.assert_array_equal(B.points, before.points)
    np.testing.assert_array_equal(G.rotation2, before_g.rotation2)
