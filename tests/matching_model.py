"""numpy restatement of tmi_ba_match_features (theia_mi355_ba.h, steps 1 to 6) in fp32, an independent float64
evaluation of the same decisions with their margins, and the inputs of the device tests (tests/test_gpu_matching.py),
which tests/test_matching_cpu.py checks for decisions that are too close to call.

The fp32 model accumulates over k with float32 arrays: numpy rounds every elementwise operation on its own, never
contracts a multiply and an add, and keeps subnormals.  It selects with a stable lexsort on (distance, index), which
has nothing in common with the device's tiling."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from theiasfm_amd import synth  # noqa: E402

MARGIN = 1e-4  # (D + 2) 2^-24 = 7.9e-6 at D = 130 bounds the fp32 sum's relative error; the margin is > 10 x that

DEFAULTS = dict(use_lowes_ratio=True, lowes_ratio=0.8, keep_only_symmetric_matches=True, min_num_feature_matches=30)


def ratio_sq(lowes_ratio) -> float:
    """(double)(float)(lowes_ratio * lowes_ratio) with the product formed in fp32."""
    r = np.float32(lowes_ratio)
    return float(np.float32(r * r))


def distances(a, b, dtype=np.float32):
    """d[i, j] = sum over ascending k of (a[i, k] - b[j, k])^2, every operation in `dtype`."""
    a = np.asarray(a, dtype=dtype)
    b = np.asarray(b, dtype=dtype)
    acc = np.zeros((a.shape[0], b.shape[0]), dtype=dtype)
    for k in range(a.shape[1]):
        t = a[:, k][:, None] - b[:, k][None, :]
        acc = acc + t * t
    return acc


def nearest_two(d):
    """Per row of d: (best distance, best column, second distance) under (distance, then lower column); -1 / inf where
    there is no such column."""
    n, m = d.shape
    best_d = np.full(n, np.inf, dtype=d.dtype)
    best_i = np.full(n, -1, dtype=np.int64)
    second_d = np.full(n, np.inf, dtype=d.dtype)
    cols = np.arange(m)
    for i in range(n if m else 0):
        order = np.lexsort((cols, d[i]))  # stable: distance, then index
        best_i[i] = order[0]
        best_d[i] = d[i, order[0]]
        if m >= 2:
            second_d[i] = d[i, order[1]]
    return best_d, best_i, second_d


def ratio_pass(best_d, best_i, second_d, num_cols, use_lowes_ratio, lowes_ratio):
    ok = best_i >= 0
    if use_lowes_ratio:
        if num_cols < 2:
            return np.zeros_like(ok)
        ok = ok & (best_d.astype(np.float64) < ratio_sq(lowes_ratio) * second_d.astype(np.float64))
    return ok


def match_pair(a, b, use_lowes_ratio=True, lowes_ratio=0.8, keep_only_symmetric_matches=True,
               min_num_feature_matches=30):
    """One pair: dict(status, num_forward, feature1, feature2, distance)."""
    d = distances(a, b)
    bd, bi, sd = nearest_two(d)
    fwd = ratio_pass(bd, bi, sd, d.shape[1], use_lowes_ratio, lowes_ratio)
    num_forward = int(fwd.sum())
    empty = dict(status=1, num_forward=num_forward, feature1=np.zeros(0, np.int32), feature2=np.zeros(0, np.int32),
                 distance=np.zeros(0, np.float32))
    if num_forward < min_num_feature_matches:
        return empty
    keep = fwd.copy()
    if keep_only_symmetric_matches:
        rd, ri, rs = nearest_two(np.ascontiguousarray(d.T))  # d(b, a) == d(a, b) in every bit
        rev = ratio_pass(rd, ri, rs, d.shape[0], use_lowes_ratio, lowes_ratio)
        for i in np.nonzero(fwd)[0]:
            j = bi[i]
            keep[i] = rev[j] and ri[j] == i
    if int(keep.sum()) < min_num_feature_matches:
        return empty
    rows = np.nonzero(keep)[0]
    return dict(status=0, num_forward=num_forward, feature1=rows.astype(np.int32), feature2=bi[rows].astype(np.int32),
                distance=bd[rows].astype(np.float32))


def match_batch(image_begin, descriptors, pair_image1, pair_image2, pairs_per_chunk=0, **options):
    """The whole call, in chunks of pairs_per_chunk pairs (0: one chunk): the arrays of lib.match_features."""
    P = len(pair_image1)
    step = pairs_per_chunk if pairs_per_chunk else max(P, 1)
    status, nfwd, begin, f1, f2, dist = [], [], [0], [], [], []
    for c0 in range(0, P, step):
        for p in range(c0, min(c0 + step, P)):
            i1, i2 = int(pair_image1[p]), int(pair_image2[p])
            r = match_pair(descriptors[image_begin[i1]:image_begin[i1 + 1]],
                           descriptors[image_begin[i2]:image_begin[i2 + 1]], **options)
            status.append(r["status"])
            nfwd.append(r["num_forward"])
            begin.append(begin[-1] + r["feature1"].shape[0])
            f1.append(r["feature1"])
            f2.append(r["feature2"])
            dist.append(r["distance"])
    cat = lambda xs, t: np.concatenate(xs).astype(t) if xs else np.zeros(0, t)  # noqa: E731
    return dict(pair_status=np.asarray(status, np.int8), pair_num_forward=np.asarray(nfwd, np.int32),
                pair_match_begin=np.asarray(begin, np.int64), feature1=cat(f1, np.int32), feature2=cat(f2, np.int32),
                distance=cat(dist, np.float32))


def reference_decisions(a, b, lowes_ratio=0.8):
    """The decisions of one direction with distances in float64: per row the best column, whether the ratio test
    passes, the relative gap of best to second best, (d1 - d0) / d1, and of d0 to ratio_sq d1,
    |d0 - ratio_sq d1| / (ratio_sq d1).  A gap whose denominator is 0 is 0; rows without a second column have gaps of
    inf."""
    d = distances(a, b, np.float64)
    bd, bi, sd = nearest_two(d)
    rs = ratio_sq(lowes_ratio)
    with np.errstate(invalid="ignore", divide="ignore"):
        gap_best = np.where(sd > 0, (sd - bd) / sd, 0.0)
        gap_ratio = np.where(sd > 0, np.abs(bd - rs * sd) / (rs * sd), 0.0)
    gap_best[np.isinf(sd)] = np.inf
    gap_ratio[np.isinf(sd)] = np.inf
    return dict(best=bi, passes=(bd < rs * sd) & (bi >= 0) & (d.shape[1] >= 2), gap_best=gap_best, gap_ratio=gap_ratio,
                best_d=bd, second_d=sd)


# ---- the inputs of the device tests --------------------------------------------------------------
SIZES = (0, 1, 2, 3, 63, 64, 65, 129, 257)
# image indices into SIZES, crossed sparsely: every size as N1 and as N2, an image in many pairs (8), pairs (i, i) and
# pairs (i, j) with (j, i)
SIZE_PAIRS = ((0, 4), (4, 0), (0, 0), (1, 1), (1, 8), (8, 1), (2, 3), (3, 2), (2, 2), (4, 5), (5, 4), (5, 6), (6, 5),
              (6, 7), (7, 6), (7, 8), (8, 7), (8, 8), (8, 4), (3, 8), (7, 7))
DIMS = (1, 3, 10, 32, 33, 128, 130, 200)  # 200: above the dimension up to which the row block stays in LDS


def _pairs(pairs):
    p = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    return p[:, 0].copy(), p[:, 1].copy()


@functools.lru_cache(maxsize=None)
def size_case(dim):
    """Images of the sizes SIZES at dimension `dim`.  dim <= 3 is integer-valued (in so few dimensions random
    descriptors are nearly equidistant); planted duplicates and ties ride along.  exact: every fp32 operation is exact."""
    integer = dim <= 3
    # every row is a noisy copy of one of 64 pool descriptors: a nearest neighbour is never a toss-up between two
    # unrelated descriptors, which among random ones happens about once in a thousand rows at the 1e-4 margin.  The
    # seeds are those for which test_matching_cpu.py finds no decision under the margin.
    seed = {10: 1110}.get(dim, 100 + dim)
    begin, desc, meta = synth.make_matching_batch(len(SIZES), SIZES, dim, seed=seed, match_share=1.0, noise=0.03,
                                                  num_duplicates=1, integer=integer, pool_size=64)
    p1, p2 = _pairs(SIZE_PAIRS)
    return dict(name=f"sizes-d{dim}", image_begin=begin, descriptors=desc, pair_image1=p1, pair_image2=p2,
                exact=integer, meta=meta)


@functools.lru_cache(maxsize=None)
def large_case():
    """The one larger pair, 2000 x 1500 x 128: every row has a true partner (a pool of 1500), so no nearest neighbour
    is a toss-up between two unrelated descriptors."""
    begin, desc, meta = synth.make_matching_batch(2, (2000, 1500), 128, seed=7, match_share=1.0, noise=0.03,
                                                  pool_size=1500)
    p1, p2 = _pairs([(0, 1)])
    return dict(name="large", image_begin=begin, descriptors=desc, pair_image1=p1, pair_image2=p2, exact=False,
                meta=meta)


@functools.lru_cache(maxsize=None)
def integer_case():
    begin, desc, meta = synth.make_matching_batch(3, (129, 65, 64), 128, seed=11, match_share=0.7, noise=0.02,
                                                  num_duplicates=2, num_ties=2, integer=True)
    p1, p2 = _pairs([(0, 1), (1, 0), (1, 2), (2, 2)])
    return dict(name="integer", image_begin=begin, descriptors=desc, pair_image1=p1, pair_image2=p2, exact=True,
                meta=meta)


@functools.lru_cache(maxsize=None)
def zero_case():
    begin = np.asarray([0, 65, 130, 133], dtype=np.int64)
    p1, p2 = _pairs([(0, 1), (1, 2), (2, 2)])
    return dict(name="zero", image_begin=begin, descriptors=np.zeros((133, 33), np.float32), pair_image1=p1,
                pair_image2=p2, exact=True, meta={})


@functools.lru_cache(maxsize=None)
def subnormal_case():
    """Magnitude 1e-20: whole multiples (0..15) of 2^-67 = 6.8e-21.  Every difference is a multiple of 2^-67, every
    square a multiple of 2^-134 below 2^-126, i.e. an fp32 SUBNORMAL, and so is every sum (at most 32 * 225 * 2^-134);
    all of them are exact.  Flushed to zero, every distance would be 0 and column 0 would win every row."""
    rng = np.random.default_rng(5)
    vals = rng.integers(0, 16, (65 + 70, 32)).astype(np.float64) * 2.0 ** -67
    begin = np.asarray([0, 65, 135], dtype=np.int64)
    p1, p2 = _pairs([(0, 1), (1, 0)])
    return dict(name="subnormal", image_begin=begin, descriptors=vals.astype(np.float32), pair_image1=p1,
                pair_image2=p2, exact=True, meta={})


@functools.lru_cache(maxsize=None)
def tile_tie_case():
    """130 columns, 4 queries.  Query 0: equal best distances at columns 5 and 100 (two column tiles of 64); query 1:
    at columns 70 and 90 (one tile); query 2: at columns 63 and 64 (the tile boundary); query 3: at columns 129 and 3
    (the last, partial tile against the first).  Each pair of columns is the query with element 0 moved by -+2^-6."""
    begin, desc, meta = synth.make_matching_batch(2, (4, 130), 32, seed=21, match_share=0.0)
    desc = desc.copy()
    e = np.float32(2.0 ** -6)
    planted = []
    for q, (lo, hi) in enumerate(((5, 100), (70, 90), (63, 64), (129, 3))):
        desc[q, 0] = np.float32(np.round(desc[q, 0] * 32.0) / 32.0)
        for col, s in ((lo, -e), (hi, e)):
            desc[4 + col] = desc[q]
            desc[4 + col, 0] = desc[q, 0] + s
        planted.append((q, 1, lo, hi))
    p1, p2 = _pairs([(0, 1), (1, 0)])
    return dict(name="tile-ties", image_begin=begin, descriptors=desc, pair_image1=p1, pair_image2=p2, exact=False,
                meta={"tie_rows": planted, "duplicate_rows": []})


@functools.lru_cache(maxsize=None)
def count_case():
    """One 65 x 64 pair for the min_num_feature_matches cases."""
    begin, desc, meta = synth.make_matching_batch(2, (65, 64), 32, seed=31, match_share=0.5, noise=0.05)
    p1, p2 = _pairs([(0, 1)])
    return dict(name="counts", image_begin=begin, descriptors=desc, pair_image1=p1, pair_image2=p2, exact=False,
                meta=meta)


def gpu_cases():
    return [size_case(d) for d in DIMS] + [large_case(), integer_case(), zero_case(), subnormal_case(),
                                           tile_tie_case(), count_case()]


def case_args(case):
    return case["image_begin"], case["descriptors"], case["pair_image1"], case["pair_image2"]


def planted_rows(case):
    """(image, row) of the descriptors that take part in a planted tie or duplicate."""
    rows = set()
    for q, m, lo, hi in case["meta"].get("tie_rows", []):
        rows.update(((0, q), (m, lo), (m, hi)))
    for m, dst, src in case["meta"].get("duplicate_rows", []):
        rows.update(((m, dst), (m, src)))
    return rows


@functools.lru_cache(maxsize=None)
def _model_cached(name, key):
    case = next(c for c in gpu_cases() if c["name"] == name)
    return match_batch(*case_args(case), **dict(key))


def model(case, **options):
    """match_batch of a case, computed once per (case, options) and shared: treat the result as read-only."""
    o = dict(DEFAULTS)
    o.update(options)
    return _model_cached(case["name"], tuple(sorted(o.items())))
