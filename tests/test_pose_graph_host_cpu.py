"""The host pieces that the five global pose estimators share (theiasfm_amd/csrc/pose_graph_host.h), compiled for the
host (tests/cpp/pose_graph_host_check.cc: its own main, under -fsanitize=address,undefined), against a few lines of
numpy written from the documented ordering -- row: ascending edge index, code edge << 1 | is_view2; lap_row: the free
neighbours sorted by (column, edge) -- at the smallest shapes that can go wrong, and the option check against the texts
the two nonlinear estimators have always returned."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

# (name, V, fixed, edges, mask); fixed = V: no view is held
STAR = 301
GRAPHS = [
    ("pair, first held", 2, 0, [(0, 1)], [1, 1]),
    ("pair, last held", 2, 1, [(0, 1)], [1, 1]),
    ("pair, none held", 2, 2, [(1, 0)], [1, 1]),
    ("path of 3, middle held", 3, 1, [(0, 1), (2, 1)], [1, 1, 1]),
    ("star, hub held", 5, 0, [(0, 1), (2, 0), (0, 3), (4, 0)], [1, 1, 1, 1, 1]),
    # the hub's row is longer than one workgroup's 256 threads
    ("star of 300 leaves, hub free", STAR, 0, [((3, v) if v % 2 else (v, 3)) for v in range(STAR) if v != 3], [1] * STAR),
    ("two components", 4, 0, [(0, 1), (3, 2)], [1, 1, 1, 1]),
    # view 2 is unmarked in the middle; view 5 is marked but its only neighbour is not: dropped from the problem
    ("subset", 6, 6, [(0, 1), (1, 2), (2, 3), (4, 3), (2, 5)], [1, 1, 0, 1, 1, 1]),
    ("no edge at either end", 5, 1, [(1, 2), (3, 2), (1, 3)], [0, 1, 1, 1, 0]),
]

# the literal texts of the parent's side_calls.h (check_nonlinear_position_arguments and the body of
# tmi_ba_estimate_global_rotations_nonlinear)
BOUND_FIELDS = ("function_tolerance", "gradient_tolerance", "parameter_tolerance", "initial_trust_region_radius",
                "max_trust_region_radius", "min_trust_region_radius", "min_relative_decrease", "min_lm_diagonal",
                "max_lm_diagonal")
TEXTS = {
    "position": {
        "robust_loss_width": "nonlinear positions: robust_loss_width is not positive and finite (the reference CHECK_GTs it)",
        "max_num_iterations": "nonlinear positions: max_num_iterations < 0",
        "bound": "nonlinear positions: a radius, tolerance or LM diagonal bound that is negative or NaN",
        "zero": "nonlinear positions: initial_trust_region_radius is 0",
    },
    "rotation": {
        "robust_loss_width": "nonlinear rotations: robust_loss_width is not positive and finite",
        "max_num_iterations": "nonlinear rotations: max_num_iterations < 0",
        "bound": "nonlinear rotations: a radius, tolerance or LM diagonal bound that is negative or NaN",
        "zero": "nonlinear rotations: initial_trust_region_radius is 0",
    },
}


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pose_graph") / "pose_graph_host_check")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    cmd = [entry._hipcc(), "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", *san,
           "-I" + os.path.join(ROOT, "theiasfm_amd", "csrc"), "-o", exe,
           os.path.join(ROOT, "tests", "cpp", "pose_graph_host_check.cc")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr

    def run(text):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
        q = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600, env=env)
        assert q.returncode == 0, q.stderr
        return q.stdout.splitlines()
    return run


def _column(v, fixed):
    return -1 if v == fixed else v - (v > fixed)


def _rows(V, fixed, edges):
    """row_ptr, row, lap_ptr, lap_row from the documented ordering."""
    row = [[(b if v == a else a, e << 1 | (v == b)) for e, (a, b) in enumerate(edges) if v in (a, b)] for v in range(V)]
    free = [v for v in range(V) if v != fixed]
    lap = [sorted((_column(nbr, fixed), code >> 1) for nbr, code in row[v] if nbr != fixed) for v in free]
    ptr = lambda lists: np.concatenate([[0], np.cumsum([len(x) for x in lists], dtype=int)]).tolist()  # noqa: E731
    flat = lambda lists: [int(x) for entries in lists for pair in entries for x in pair]  # noqa: E731
    return ptr(row), flat(row), ptr(lap), flat(lap)


def _components(V, edges):
    """The smallest view of every view's component."""
    root = np.arange(V)
    for _ in range(V):
        for a, b in edges:
            root[a] = root[b] = min(root[a], root[b])
    return root


def _subset(V, edges, mask):
    kept = [e for e, (a, b) in enumerate(edges) if mask is None or (mask[a] and mask[b])]
    view_of = sorted({v for e in kept for v in edges[e]})
    index = [view_of.index(v) if v in view_of else -1 for v in range(V)]
    return index, view_of, kept, [index[edges[e][0]] for e in kept], [index[edges[e][1]] for e in kept]


def _ints(line, name):
    words = line.split()
    assert words[0] == name, line
    return [int(w) for w in words[1:]]


def _groups(line, name):
    assert line.startswith(name + " "), line
    return [[int(w) for w in part.split()] for part in line[len(name) + 1:].split("|")]


def test_rows_components_subsets_and_the_free_vector(host_check):
    text = "".join("graph %d %d %d %s %s\n" % (V, len(edges), fixed, " ".join("%d %d" % e for e in edges),
                                               " ".join(map(str, mask))) for _, V, fixed, edges, mask in GRAPHS)
    lines = host_check(text)
    assert len(lines) == 11 * len(GRAPHS)
    for g, (name, V, fixed, edges, mask) in enumerate(GRAPHS):
        out = lines[11 * g:11 * g + 11]
        row_ptr, row, lap_ptr, lap_row = _rows(V, fixed, edges)
        assert _ints(out[0], "row_ptr") == row_ptr, name
        assert _ints(out[1], "row") == row, name
        assert _ints(out[2], "lap_ptr") == lap_ptr, name
        assert _ints(out[3], "lap_row") == lap_row, name
        root = _components(V, edges)
        comp = _ints(out[4], "components")
        assert comp[0] == len(set(root.tolist())), name
        assert comp[1:1 + V] == root.tolist(), name
        assert comp[1 + V:] == [int((root == root[v]).all()) for v in range(V)], name
        assert _groups(out[5], "masked") == [list(x) for x in _subset(V, edges, mask)], name
        assert _groups(out[6], "unmasked") == [list(x) for x in _subset(V, edges, None)], name
        table = [100 * v + k for v in range(V) for k in range(3)]
        assert _ints(out[7], "gathered") == [x for v in range(V) if v != fixed for x in table[3 * v:3 * v + 3]], name
        assert _ints(out[8], "scattered") == [x if i // 3 != fixed else -1 for i, x in enumerate(table)], name
        free = _subset(V, edges, mask)[1][1:]
        assert _ints(out[9], "gathered_subset") == [x for v in free for x in table[3 * v:3 * v + 3]], name
        assert _ints(out[10], "scattered_subset") == [x if i // 3 in free else -1 for i, x in enumerate(table)], name
    # what the shapes are there for
    assert _rows(5, 0, GRAPHS[4][3])[3] == []  # the hub held: every lap list is empty
    assert max(np.diff(_rows(STAR, 0, GRAPHS[5][3])[0])) == 300 > 256
    assert len(set(_components(4, GRAPHS[6][3]).tolist())) == 2
    assert _subset(6, GRAPHS[7][3], GRAPHS[7][4])[1] == [0, 1, 3, 4]


def test_the_option_check_returns_the_texts_it_always_did(host_check):
    lines = host_check("options\n")
    got = {}
    for line in lines:
        head, _, text = line.partition(":")
        got[tuple(head.split())] = text[1:]
    fields = ("robust_loss_width", "max_num_iterations") + BOUND_FIELDS
    assert len(got) == 2 * (2 + 2 * len(fields) - 1)  # (max_num_iterations is an integer: no NaN)
    for which, texts in TEXTS.items():
        assert got[(which, "none", "0")] == ""
        assert got[(which, "initial_trust_region_radius", "0")] == texts["zero"]
        for field in fields:
            want = texts["bound"] if field in BOUND_FIELDS else texts[field]
            assert got[(which, field, "-1")] == want, (which, field)
            if field != "max_num_iterations":
                assert got[(which, field, "nan")] == want, (which, field)
