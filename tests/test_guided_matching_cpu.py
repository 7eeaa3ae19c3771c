"""tmi_ba_guided_epipolar_match without a device: the model (tests/guided_matching_model.py) on the device tests'
inputs (tests/guided_matching_cases.py), the margins of every decision the fp64 geometry feeds, the argument errors
through the real library (they return before the device is looked for) and TMI_BA_ERR_NO_DEVICE."""
import ctypes as C

import numpy as np
import pytest

import guided_matching_cases as gc
import guided_matching_model as gm
from theiasfm_amd import abi, lib

CASES = gc.cases()
IDS = [c["name"] for c in CASES]


def test_abi_mirrors_and_defaults():
    L = lib.load()
    assert "tmi_ba_guided_epipolar_match" in lib.EXPORTS and "tmi_ba_guided_match_options_init" in lib.EXPORTS
    c = abi.CGuidedMatchOptions()
    L.tmi_ba_guided_match_options_init(C.byref(c))
    d = abi.guided_match_options()
    for name, _ in abi.CGuidedMatchOptions._fields_[:5]:
        assert getattr(c, name) == getattr(d, name), name
    assert (c.guided_matching_max_distance_pixels, c.lowes_ratio, c.min_num_candidates, c.device, c.seed) == \
        (2.0, 0.8, 50, -1, 0) and list(c.reserved) == [0, 0]
    assert C.sizeof(abi.CGuidedMatchOptions) == 40 and C.sizeof(abi.CGuidedMatchSummary) == 64


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_model_on_the_cases(case):
    ref = gc.model(case)
    a = gc.case_args(case)
    assert ref["pair_status"].tolist() == [0, 0, 0, 0, 1, 0, 0]
    for p, r in enumerate(ref["pairs"]):
        m = slice(a[6][p], a[6][p + 1])
        # no added match touches a matched image-1 feature; every added feature is in a group
        assert not (set(r["feature1"].tolist()) & set(a[7][m].tolist()))
        assert (r["feature_group"][r["feature1"]] >= 0).all()
        assert all(25 < len(c) for c in r["group_candidates"])  # (draws of the fill may coincide)
        # the added matches come in ascending (group, position in the group)
        order = [(int(r["feature_group"][f]), r["group_features"][r["feature_group"][f]].index(f)) for f in r["feature1"]]
        assert order == sorted(order)
    # the general pair: of the held-out true matches whose line meets the box at least 90 % come back
    r, held = ref["pairs"][0], case["held_out"][0]
    with_line = [(int(f1), int(f2)) for f1, f2 in held if r["feature_group"][f1] >= 0]
    added = set(zip(r["feature1"].tolist(), r["feature2"].tolist()))
    got = sum(1 for h in with_line if h in added)
    print(f"{case['name']}: general pair recovers {got} of {len(with_line)} held-out matches with a line")
    assert len(with_line) >= 100 and got >= 0.9 * len(with_line)
    # the epipole of pair 1 is inside image 2; pairs 2 and 3 have exactly horizontal and exactly vertical lines
    F = case["fundamental_matrix"][1].reshape(3, 3)
    e = np.linalg.svd(F.T)[2][-1]
    assert 0 < e[0] / e[2] < 2 * gc.CX and 0 < e[1] / e[2] < 2 * gc.CY
    ends = ref["group_endpoints"]
    rows = ref["pair_row"]
    for p, (first, second) in ((2, (1, 3)), (3, (0, 2))):  # a group's lines end within a group's width of each other
        g = ends[rows[p]:rows[p] + ref["pair_num_groups"][p]]
        assert len(g) > 20 and (np.abs(g[:, first] - g[:, second]) < 4.0).all()
    assert ref["pair_num_groups"][4] == 0 and ref["pair_num_groups"][5] == 0
    # the sparse pair: every group needs the fill
    assert all(len(c) <= 50 for c in ref["pairs"][6]["group_candidates"]) and ref["pair_num_groups"][6] > 5


@pytest.mark.parametrize("case,options", [(c, {}) for c in CASES] + [(CASES[0], gc.OTHER_OPTIONS)],
                         ids=IDS + [IDS[0] + "-other-options"])
def test_no_decision_is_too_close_to_call(case, options):
    """Every decision the fp64 geometry feeds (the two-endpoint tests, the truncations, the group split, the number of
    steps, the cells of features and of samples, the closest centre) and the fp32 ratio test and nearest neighbour.  A
    decision is RISKY when it lies within gm.MARGIN (gm.RATIO_MARGIN for the fp32 ones) of its boundary, or is a tie
    whose operands are not exact.  Integer endpoints and c = 2 make some unavoidable: the last sample of a walk is the
    group's integer endpoint up to rounding, which is a cell border of two of the four grids.  So every risky decision
    is turned, and none may change an output (the seeds of the cases are chosen so): those of the walks are examined on the spot (the cell the other outcome
    would take must leave the group's candidate set as it is), the others by running the pair again with that one
    decision flipped.  A risky ratio test or nearest neighbour always counts as changing an output."""
    ref = gc.model(case, **options)
    a = gc.case_args(case)
    n = gc.NUM_POINTS + gc.NUM_OWN
    o = dict(gm.DEFAULTS)
    o.update(options)
    total = risky = affecting = 0
    for p, r in enumerate(ref["pairs"]):
        D = r["decisions"]
        total += D.count
        risky += len(D.flagged) + sum(D.walk_risky.values())
        i1, i2 = gc.PAIRS[p]
        m = slice(a[6][p], a[6][p + 1])
        for g, step, kind in D.walk_affecting:
            affecting += 1
            print(f"  {case['name']} pair {p}: {kind} at step {step} of group {g} CHANGES THE CANDIDATES")
        for i, kind, gap in D.flagged:
            same = kind not in ("ratio", "nearest")
            if same:
                alt = gm.guided_pair(a[1][i1 * n:(i1 + 1) * n], a[2][i1 * n:(i1 + 1) * n], a[1][i2 * n:(i2 + 1) * n],
                                     a[2][i2 * n:(i2 + 1) * n], a[5][p], a[7][m], a[8][m], stream=p, flip=i, **o)
                same = all(alt[k].tobytes() == r[k].tobytes() for k in (
                    "feature_group", "group_endpoints", "group_num_candidates", "feature1", "feature2", "distance"))
            affecting += 0 if same else 1
            print(f"  {case['name']} pair {p}: {kind} gap {gap:.3g} {'changes nothing' if same else 'CHANGES AN OUTPUT'}")
        print(f"  {case['name']} pair {p}: risky in the walks {D.walk_risky}, elsewhere {len(D.flagged)}")
    print(f"{case['name']}: {total} decisions, {risky} risky, {affecting} of them change an output")
    assert affecting == 0


def _call(case, **kw):
    return lib.guided_epipolar_match(*gc.case_args(case), **kw)


def test_argument_errors_come_before_the_device():
    case = CASES[0]
    a = list(gc.case_args(case))

    def invalid(args=None, **kw):
        with pytest.raises(lib.EngineError) as e:
            lib.guided_epipolar_match(*(args or a), **kw)
        assert e.value.status == abi.ERR_INVALID_ARGUMENT, e.value

    for o in (dict(guided_matching_max_distance_pixels=0.0), dict(guided_matching_max_distance_pixels=-1.0),
              dict(guided_matching_max_distance_pixels=float("nan")), dict(lowes_ratio=float("inf")),
              dict(lowes_ratio=float("nan")), dict(min_num_candidates=-1), dict(min_num_candidates=65)):
        invalid(options=abi.guided_match_options(**o))
    invalid(added_capacity=-1)
    # a positive distance below 1/16 is a valid argument outside the supported range
    for tiny in (0.01, 0.0624):
        with pytest.raises(lib.EngineError) as e:
            lib.guided_epipolar_match(*a, options=abi.guided_match_options(guided_matching_max_distance_pixels=tiny))
        assert e.value.status == abi.ERR_UNSUPPORTED

    def changed(i, f):
        b = list(a)
        b[i] = f(np.array(a[i], copy=True))
        return b

    def put(index, value):
        def f(x):
            x[index] = value
            return x
        return f

    invalid(changed(3, put(0, len(a[0]) - 1)))                                # image index out of range
    invalid(changed(4, put(2, -1)))
    invalid(changed(7, put(0, gc.NUM_POINTS + gc.NUM_OWN)))                   # match index out of range
    invalid(changed(8, put(5, -1)))
    mb = np.array(a[6], copy=True)
    mb[2], mb[3] = mb[3], mb[2]
    invalid(changed(6, lambda x: mb))                                         # pair_match_begin decreases
    # dim <= 0, null pointers and an image above the bitmap cap, through the raw entry point
    L = lib.load()
    o = abi.guided_match_options()
    s = abi.CGuidedMatchSummary()
    begin = np.array([0, 4, 8], np.int64)
    desc, keys = np.zeros((8, 4), np.float32), np.zeros((8, 2))
    p1, p2, F = np.array([0], np.int32), np.array([1], np.int32), np.ones(9)
    mbeg = np.zeros(2, np.int64)
    st, ng, ab = np.zeros(1, np.int8), np.zeros(1, np.int32), np.zeros(2, np.int64)

    def raw(opt=C.byref(o), ib=begin, d=desc, dim=4, k=keys, np_=1, a1=p1, fm=F, mbegin=mbeg, cap=0, summ=C.byref(s),
            num_images=2, abegin=ab):
        ptr = lambda x: None if x is None else x.ctypes.data  # noqa: E731
        return L.tmi_ba_guided_epipolar_match(opt, num_images, ptr(ib), ptr(d), dim, ptr(k), np_, ptr(a1), ptr(p2),
                                              ptr(fm), ptr(mbegin), None, None, None, None, cap, ptr(st), ptr(ng),
                                              ptr(abegin), None, None, None, None, None, None, summ)

    assert raw() in (0, 2)  # OK, or NO_DEVICE: the arguments are fine
    for kw in (dict(opt=None), dict(summ=None), dict(ib=None), dict(d=None), dict(k=None), dict(dim=0), dict(dim=-3),
               dict(np_=-1), dict(num_images=-1), dict(a1=None), dict(fm=None), dict(mbegin=None), dict(abegin=None),
               dict(cap=4), dict(ib=np.array([0, 4, 4 + 131073], np.int64)), dict(ib=np.array([0, 4, 2], np.int64)),
               dict(ib=np.array([1, 4, 8], np.int64)), dict(mbegin=np.array([0, -1], np.int64)),
               dict(mbegin=np.array([1, 1], np.int64))):
        assert raw(**kw) == abi.ERR_INVALID_ARGUMENT, kw


def test_without_a_device_the_call_says_so():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is visible")
    with pytest.raises(lib.EngineError) as e:
        _call(CASES[0])
    assert e.value.status == 2 and abi.STATUS_NAMES[2] == "NO_DEVICE"
