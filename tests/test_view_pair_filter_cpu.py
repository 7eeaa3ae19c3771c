"""The view-pair filters without a GPU: the CPU model (tests/view_pair_filter_model.py) on the reference's own test
cases and on graphs whose answer is known by construction, the argument checks of
tmi_ba_filter_view_pairs_from_relative_translation and tmi_ba_filter_view_pairs_from_orientation (status 1 before the
device is looked for, status 2 for a valid batch where there is no device), and the Python side of the ABI."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402
import view_pair_filter_model as model  # noqa: E402
from theiasfm_amd import abi, lib, synth  # noqa: E402

INVALID_ARGUMENT, NO_DEVICE = 1, 2


@pytest.fixture(scope="module")
def L():
    entry.build_engine()
    return lib.load()


# ---- the reference's cases on the model ----------------------------------------------------------------------------
@pytest.mark.parametrize("seed", model.LINE_SEEDS)
def test_line_test_leaves_the_three_valid_edges(seed):
    V, v1, v2, pos = model.line_case()
    r = model.filter_from_relative_translation(V, v1, v2, pos, model.draw_axes(pos, 48, seed), tolerance=0.1)
    assert r.removed.tolist() == [0, 0, 0, 1]


@pytest.mark.parametrize("name,views,valid,invalid,seeds", model.REFERENCE_CASES, ids=[c[0] for c in model.REFERENCE_CASES])
def test_reference_cases_keep_at_least_the_valid_count(name, views, valid, invalid, seeds):
    for seed in seeds:
        B, _ = synth.make_view_pair_batch(views, valid, invalid, seed)
        assert B.num_pairs == valid + invalid
        t, _ = model.rotate_translations(B.view_rotation, B.pair_view1, B.pair_position2)
        r = model.filter_from_relative_translation(views, B.pair_view1, B.pair_view2, None, model.draw_axes(t, 48, seed),
                                                   translation=t)
        kept = int((r.removed == 0).sum())
        print(name, seed, "kept", kept, "of", B.num_pairs)
        assert kept >= valid, (name, seed)


# ---- by construction -------------------------------------------------------------------------------------------------
def test_consistent_translations_have_zero_bad_weight_for_every_axis():
    B, pos = synth.make_view_pair_batch(25, 80, 0, 11)
    rng = np.random.default_rng(4)
    axes = rng.normal(size=(16, 3))
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    d = pos[B.pair_view2] - pos[B.pair_view1]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = model.filter_from_relative_translation(25, B.pair_view1, B.pair_view2, d, axes)
    assert (r.contribution == 0.0).all() and (r.bad_weight == 0.0).all() and not r.removed.any()
    # and through the rotation stage: the translations of the batch are those directions up to round-off, and a
    # projection that round-off leaves on the wrong side of zero has a weight of that size
    r = model.filter_from_relative_translation(25, B.pair_view1, B.pair_view2, B.pair_position2, axes,
                                               view_rotation=B.view_rotation)
    assert np.abs(r.translation - d).max() < 1e-14 and r.bad_weight.max() < 1e-13 and not r.removed.any()


def test_one_reversed_edge_in_a_path_is_the_only_positive_weight():
    """Views 0 .. 8 on a line, the path edges (i, i + 1) pointing along +x, and the edge (0, 8) that closes the ring
    pointing along -x, against the line.  (A reversed edge of the path itself contradicts nothing: the graph stays
    acyclic and every order of an acyclic graph is consistent.)  Every weight of an iteration is the same, so every
    score ties, view 0 goes first by the smallest-index rule, and then there is always a source: the order is
    0 .. 8 and the closing edge alone is bad."""
    n = 9
    v1 = np.concatenate([np.arange(n - 1), [0]]).astype(np.int32)
    v2 = np.concatenate([np.arange(1, n), [n - 1]]).astype(np.int32)
    t = np.tile([1.0, 0.0, 0.0], (n, 1))
    t[n - 1] = [-1.0, 0.0, 0.0]
    axes = np.array([[1.0, 0, 0], [0.6, 0.8, 0.0], [0.6, 0.0, -0.8]])
    r = model.filter_from_relative_translation(n, v1, v2, t, axes)
    assert (r.order == np.arange(n)).all()
    assert (r.bad_weight[:n - 1] == 0.0).all() and r.bad_weight[n - 1] == (1.0 + 0.6) + 0.6


def test_order_rules():
    # all scores tie on a cycle of equal weights: the smallest index goes first, then sources appear one by one
    v1 = np.array([0, 1, 2], np.int32)
    v2 = np.array([1, 2, 0], np.int32)
    assert model.order_from_projections(4, v1, v2, np.array([1.0, 1.0, 1.0])).tolist() == [0, 1, 2, -1]
    # a zero projection is an incoming node at view1: view2 is the source
    assert model.order_from_projections(2, v1[:1], v2[:1], np.array([0.0])).tolist() == [1, 0]
    assert model.order_from_projections(2, v1[:1], v2[:1], np.array([0.5])).tolist() == [0, 1]


def test_orientation_model_on_a_consistent_scene():
    B, _ = synth.make_view_pair_batch(12, 40, 9, 3)
    removed, angles, spread = model.filter_from_orientation(B.view_rotation, B.pair_view1, B.pair_view2,
                                                            B.pair_rotation2, 2.0)
    assert angles[:40].max() < 1e-7 and not removed[:40].any()  # (atan2 near 0 keeps the sine's absolute accuracy)
    assert removed[40:].all() and spread < 1e-13
    assert not model.filter_from_orientation(B.view_rotation, B.pair_view1, B.pair_view2, B.pair_rotation2, 180.0)[0].any()


# ---- the ABI ---------------------------------------------------------------------------------------------------------
def test_symbols_are_exported(L):
    for name in ("tmi_ba_translation_filter_options_init", "tmi_ba_filter_view_pairs_from_relative_translation",
                 "tmi_ba_filter_view_pairs_from_orientation"):
        assert name in lib.EXPORTS and hasattr(L, name)
    o = abi.CTranslationFilterOptions()
    L.tmi_ba_translation_filter_options_init(C.byref(o))
    d = abi.translation_filter_options()
    assert (o.num_iterations, o.translation_projection_tolerance, o.seed) == (48, 0.08, 0) == \
        (d.num_iterations, d.translation_projection_tolerance, d.seed)


def _valid():
    return synth.make_view_pair_batch(6, 9, 2, 1)[0]


def _translation(L, cb, options=None, axes=None, axes_given=0, summary=True):
    o = options if options is not None else abi.translation_filter_options()
    s = abi.CViewPairFilterSummary()
    return L.tmi_ba_filter_view_pairs_from_relative_translation(
        None if cb is None else C.byref(cb), C.byref(o), None if axes is None else axes.ctypes.data, axes_given, -1,
        None, None, None, None, C.byref(s) if summary else None)


def _orientation(L, cb, degrees=5.0, summary=True):
    s = abi.CViewPairFilterSummary()
    return L.tmi_ba_filter_view_pairs_from_orientation(None if cb is None else C.byref(cb), degrees, -1, None, None,
                                                       C.byref(s) if summary else None)


def _null(cb, name):
    setattr(cb, name, C.cast(None, type(getattr(cb, name))))


def _set(name, index, value):
    def edit(B, cb):
        getattr(B, name).reshape(-1)[index] = value
    return edit


# edits of a valid batch that both calls must refuse
BAD_BATCHES = {
    "negative num_views": lambda B, cb: setattr(cb, "num_views", -1),
    "negative num_pairs": lambda B, cb: setattr(cb, "num_pairs", -3),
    "no pair_view1": lambda B, cb: _null(cb, "pair_view1"),
    "no pair_view2": lambda B, cb: _null(cb, "pair_view2"),
    "view index too large": _set("pair_view2", 1, 6),
    "view index negative": _set("pair_view1", 0, -1),
    "view paired with itself": _set("pair_view2", 2, 2),       # edge 2 is (2, 3)
    "non-finite view_rotation": _set("view_rotation", 4, np.nan),
}


def _repeat_pair(B, cb):
    B.pair_view1[-1], B.pair_view2[-1] = B.pair_view2[0], B.pair_view1[0]  # the first edge again, reversed


BAD_BATCHES["repeated unordered pair"] = _repeat_pair


def test_argument_errors_come_before_the_device(L):
    """Each of these is TMI_BA_ERR_INVALID_ARGUMENT (1), never TMI_BA_ERR_NO_DEVICE (2), with a message."""
    def check(call, name, edit, **kw):
        B = _valid()
        cb = B.as_c()
        edit(B, cb)
        assert call(L, cb, **kw) == INVALID_ARGUMENT, name
        assert L.tmi_ba_last_error(), name

    for name, edit in BAD_BATCHES.items():
        check(_translation, name, edit)
        check(_orientation, name, edit)
    check(_translation, "no pair_position2", lambda B, cb: _null(cb, "pair_position2"))
    check(_translation, "non-finite position", _set("pair_position2", 7, np.inf))
    check(_orientation, "no pair_rotation2", lambda B, cb: _null(cb, "pair_rotation2"))
    check(_orientation, "no view_rotation", lambda B, cb: _null(cb, "view_rotation"))
    check(_orientation, "non-finite rotation_2", _set("pair_rotation2", 2, np.nan))
    check(_orientation, "negative threshold", lambda B, cb: None, degrees=-1e-3)
    check(_orientation, "NaN threshold", lambda B, cb: None, degrees=float("nan"))
    for k in (0, -4):
        check(_translation, "num_iterations < 1", lambda B, cb: None, options=abi.translation_filter_options(num_iterations=k))
    bad_axes = np.ones((48, 3))
    bad_axes[17, 1] = np.nan
    check(_translation, "non-finite given axis", lambda B, cb: None, axes=bad_axes, axes_given=1)
    check(_translation, "axes_given without axes", lambda B, cb: None, axes=None, axes_given=1)
    # one edge: the variance is undefined unless the axes are given
    one = abi.ViewPairBatch(np.zeros((2, 3)), [0], [1], None, [[1.0, 0, 0]])
    assert _translation(L, one.as_c()) == INVALID_ARGUMENT
    for call in (_translation, _orientation):
        assert call(L, None) == INVALID_ARGUMENT
        assert call(L, _valid().as_c(), summary=False) == INVALID_ARGUMENT


def test_a_valid_batch_reaches_the_device(L):
    """Without a device a valid batch is TMI_BA_ERR_NO_DEVICE (2) and nothing is written; with one it is OK."""
    want = 0 if L.tmi_ba_device_count() > 0 else NO_DEVICE
    B = _valid()
    keep = [B, abi.ViewPairBatch(np.zeros((2, 3)), [0], [1], None, [[1.0, 0, 0]]), np.array([[0.0, 0.0, 1.0]] * 48)]
    assert _translation(L, B.as_c()) == want
    assert _orientation(L, B.as_c()) == want
    assert _orientation(L, B.as_c(), degrees=0.0) == want
    assert _translation(L, keep[1].as_c(), axes=keep[2], axes_given=1) == want  # one edge with given axes is valid
    G = B.copy()
    G.view_rotation = None  # global-frame translations
    assert _translation(L, G.as_c()) == want
    if want == NO_DEVICE:
        with pytest.raises(lib.EngineError) as e:
            lib.filter_view_pairs_from_relative_translation(B)
        assert e.value.status == NO_DEVICE
        with pytest.raises(lib.EngineError) as e:
            lib.filter_view_pairs_from_orientation(B, 5.0)
        assert e.value.status == NO_DEVICE


def test_batch_copy_is_deep_and_defaults():
    B = _valid()
    Cp = B.copy()
    for name in ("view_rotation", "pair_view1", "pair_view2", "pair_rotation2", "pair_position2"):
        a, b = getattr(B, name), getattr(Cp, name)
        assert a is not b and not np.shares_memory(a, b) and (a == b).all(), name
    G = abi.ViewPairBatch(None, [0, 3], [1, 2], None, np.ones((2, 3)))
    assert G.num_views == 4 and G.as_c().num_views == 4 and not G.as_c().view_rotation
    assert abi.ViewPairBatch(None, [0], [1], num_views=9).copy().num_views == 9


def test_struct_layout_matches_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "theia_mi355_ba.h"\n'
        'int main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(tmi_ba_view_pair_batch),'
        "offsetof(tmi_ba_view_pair_batch, num_pairs), offsetof(tmi_ba_view_pair_batch, pair_position2),"
        "sizeof(tmi_ba_translation_filter_options), offsetof(tmi_ba_translation_filter_options, seed),"
        "sizeof(tmi_ba_view_pair_filter_summary), offsetof(tmi_ba_view_pair_filter_summary, num_views_ordered),"
        "offsetof(tmi_ba_view_pair_filter_summary, kernel_seconds));return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    T, O, S = abi.CViewPairBatch, abi.CTranslationFilterOptions, abi.CViewPairFilterSummary
    assert got == [C.sizeof(T), T.num_pairs.offset, T.pair_position2.offset, C.sizeof(O), O.seed.offset, C.sizeof(S),
                   S.num_views_ordered.offset, S.kernel_seconds.offset]
