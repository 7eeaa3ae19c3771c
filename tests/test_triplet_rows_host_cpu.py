"""The three host builders of the linear position estimator (theiasfm_amd/csrc/pose_graph_host.h:
build_sorted_adjacency, build_view_tracks, build_triplet_rows), compiled for the host
(tests/cpp/triplet_rows_host_check.cc: its own main, under -fsanitize=address,undefined), against a few lines of brute
force written from the documented ordering, at the shapes where the index arithmetic can go wrong: a hub, empty rows at
either end, a held view that is not view 0, a repeated track, no triplet at all."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("triplet_rows") / "triplet_rows_host_check")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    cmd = [entry._hipcc(), "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", *san,
           "-I" + os.path.join(ROOT, "theiasfm_amd", "csrc"), "-o", exe,
           os.path.join(ROOT, "tests", "cpp", "triplet_rows_host_check.cc")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr

    def run(text):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
        q = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600, env=env)
        assert q.returncode == 0, q.stderr
        out = {}
        for line in q.stdout.splitlines():
            words = line.split()
            out[words[0]] = [int(w) for w in words[1:]]
        return out
    return run


def _ptr(lists):
    ptr = [0]
    for x in lists:
        ptr.append(ptr[-1] + len(x))
    return ptr


def _flat(lists):
    return [int(x) for entries in lists for item in entries for x in item]


HUB = 300
ADJACENCY = [
    ("triangle", 3, [(0, 1), (1, 2), (0, 2)]),
    ("empty rows at both ends", 6, [(2, 3), (1, 3), (1, 2)]),
    # the hub's row is longer than a workgroup; the edges come in an order that is not the neighbours'
    ("hub", HUB + 1, [(0, v) for v in range(HUB, 0, -1)] + [(v, v + 1) for v in range(1, HUB)]),
    ("one edge", 2, [(0, 1)]),
]


@pytest.mark.parametrize("name,V,edges", ADJACENCY, ids=[a[0] for a in ADJACENCY])
def test_sorted_adjacency(host_check, name, V, edges):
    out = host_check("adjacency %d %d %s\n" % (V, len(edges), " ".join("%d %d" % e for e in edges)))
    rows = [sorted((b if v == a else a, e) for e, (a, b) in enumerate(edges) if v in (a, b)) for v in range(V)]
    assert out["ptr"] == _ptr(rows)
    assert out["adj"] == _flat(rows)
    assert out["owner"] == [v for v in range(V) for _ in rows[v]]


TRACKS = [
    ("unsorted", 3, [(2, 5), (0, 9), (2, 1), (0, 3), (2, 3), (0, 4)]),
    ("views without a feature", 5, [(3, 7), (1, 7), (3, 2)]),
    ("a repeated track", 2, [(1, 4), (0, 4), (1, 8), (1, 4)]),
    ("the same track in two views is no repeat", 2, [(0, 4), (1, 4)]),
    ("nothing", 3, []),
]


@pytest.mark.parametrize("name,V,obs", TRACKS, ids=[t[0] for t in TRACKS])
def test_view_tracks(host_check, name, V, obs):
    out = host_check("tracks %d %d %s\n" % (V, len(obs), " ".join("%d %d" % o for o in obs)))
    rows = [sorted((t, i) for i, (v, t) in enumerate(obs) if v == view) for view in range(V)]
    assert out["ptr"] == _ptr(rows)
    assert out["track"] == [t for row in rows for t, _ in row]
    assert out["obs"] == [i for row in rows for _, i in row]
    assert out["repeated"] == [int(any(len({t for t, _ in row}) < len(row) for row in rows))]


WHEEL = [(0, i, i + 1) for i in range(1, 81)]
TRIPLETS = [
    ("one triplet", 3, [(0, 1, 2)]),
    ("two sharing a pair", 4, [(0, 1, 2), (0, 1, 3)]),
    # the held view is view 5, views 0 .. 4 and 9 are not estimated
    ("held view is not view 0", 10, [(5, 6, 7), (6, 7, 8)]),
    ("a hub in 80 triplets", 82, WHEEL),
    ("the hub is the last view", 82, [(i, i + 1, 81) for i in range(0, 80)]),
    ("no triplet", 4, []),
]


@pytest.mark.parametrize("name,V,triplets", TRIPLETS, ids=[t[0] for t in TRIPLETS])
def test_triplet_rows(host_check, name, V, triplets):
    out = host_check("triplets %d %d %s\n" % (V, len(triplets), " ".join("%d %d %d" % t for t in triplets)))
    views = sorted({v for t in triplets for v in t})
    column = {v: i - 1 for i, v in enumerate(views)}
    assert out["views"] == views
    assert out["view_column"] == [column.get(v, -2) for v in range(V)]
    assert out["view_count"] == [sum(v in t for t in triplets) for v in range(V)]
    assert out["column"] == [column[v] for t in triplets for v in t]
    columns = max(0, len(views) - 1)
    entries = [[(c, s) for c, t in enumerate(triplets) for s in range(3) if column[t[s]] == p] for p in range(columns)]
    assert out["view_ptr"] == _ptr(entries)
    assert out["view_entry"] == _flat(entries)
    # every (row column, column column) with a common triplet, ascending; its triplets ascending
    blocks, pq = [], []
    for p in range(columns):
        for q in range(columns):
            ent = [(c, 3 * i + j) for c, t in enumerate(triplets) for i in range(3) for j in range(3)
                   if column[t[i]] == p and column[t[j]] == q]
            if ent:
                blocks.append(ent)
                pq.append((p, q))
    assert out["block_ptr"] == _ptr(blocks)
    assert out["block_pq"] == _flat([pq])
    assert out["block_entry"] == _flat(blocks)
    if name == "a hub in 80 triplets":
        assert out["view_column"][0] == -1 and max(out["view_count"]) == 80  # the hub is held: none of its blocks exist
    if name == "the hub is the last view":
        assert len(entries[-1]) == 80  # a free hub: a row of 80 entries, a diagonal block of 80
    if name == "held view is not view 0":
        assert out["view_column"] == [-2] * 5 + [-1, 0, 1, 2, -2]
